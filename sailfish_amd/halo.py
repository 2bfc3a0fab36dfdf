"""Halo set-up of a SubdomainRunner: which scheme carries what crosses the faces of a subdomain, its links (one
subdomain_connection.Link per neighbour and kind), their device buffers and pack / unpack kernels.

    IndexListHalo   populations (and, for the non-local models, macroscopic fields) gathered / scattered through index
                    lists by pack / unpack kernels: any decomposition
    FaceBufferHalo  1-D decompositions along x, single fluid: dense x-face buffers the sweep itself writes / reads
                    (xface.XFaceHalo), moved in pieces as the z-chunks of the sweep complete (xface.ChunkPlan)
    PlaneHalo       1-D decompositions along x, Shan-Chen models: dense planes of populations and densities the two
                    kernels of a step write / read (xface.NNPlanes)

All of them offer `links`, `macro_links`, `messages(kind, parity)`, `reset()`, `materialise()`; the runner picks one in
make() and writes its step program against that surface.  Every link has two buffers per direction, [parity of the
step]; the index-list schemes alias one buffer for both unless the transport is zero-copy (connector.PeerConnector).
"""
import numpy as np

from sailfish_amd import subdomain_connection, xface
from sailfish_amd.subdomain_connection import Link


def allocate(connector, runner, kind, links, separate):
    """send_bufs / recv_bufs [parity] of every link of `links` ({neighbour id: link}, n_send / n_recv filled in) for the
    exchange `kind` ('dist' | 'macro').  Zero-copy connectors: the receive buffers are mine, two sets, and my send buffers
    ARE the neighbours' receive buffers, known after the collective resolve() -- which every rank reaches exactly once per
    call, whatever its links, so every rank calls this the same number of times in the same order ('dist' before
    'macro').  Other connectors: one buffer per direction that serves both parities, or two where the parities are
    `separate` (planes that are written while the other set is still being read)."""
    dtype = runner.float
    order = sorted(links)
    if getattr(connector, 'zero_copy', False):
        for nid in order:
            links[nid].recv_bufs = [connector.alloc_recv(runner, kind, nid, par, links[nid].n_recv, dtype) for par in (0, 1)]
        connector.resolve(runner)
        for nid in order:
            links[nid].send_bufs = [connector.send_addr(runner, kind, nid, par) for par in (0, 1)]
        return
    for nid in order:
        link = links[nid]
        if separate:
            link.send_bufs = [connector.alloc_buffer(runner, link.n_send, dtype) for _ in (0, 1)]
            link.recv_bufs = [connector.alloc_buffer(runner, link.n_recv, dtype) for _ in (0, 1)]
        else:
            link.send_bufs = [connector.alloc_buffer(runner, link.n_send, dtype)] * 2
            link.recv_bufs = [connector.alloc_buffer(runner, link.n_recv, dtype)] * 2


def face_layout(link, n, isz):
    """[(parity, face, send address, receive address)] of a face link whose buffers hold `n` elements of `isz` bytes per
    face: I send [through my low face | through my high face] (the faces that lead to this neighbour); the neighbour does
    the same, and what it sends through its high face enters through my low one -- so its buffer read from here is [my
    high-face input | my low-face input], my own order reversed."""
    out = []
    last = len(link.faces) - 1
    for par in (0, 1):
        for k, face in enumerate(link.faces):
            out.append((par, face, link.send_bufs[par] + k * n * isz, link.recv_bufs[par] + (last - k) * n * isz))
    return out


def face_links(spec, count):
    """{neighbour id: Link} of a subdomain connected through its x faces only, `count` elements per face."""
    faces = {}
    for face, nid in sorted(spec.connecting_subdomains()):
        faces.setdefault(nid, []).append(xface.LOW if face == spec.X_LOW else xface.HIGH)
    return dict((nid, Link(nid, faces=sorted(f), n_send=count * len(f), n_recv=count * len(f))) for nid, f in faces.items())


def x_slabs_line_up(runner):
    """A 1-D decomposition along x whose slabs share their y / z extent (same answer in every runner)."""
    local = runner._local_periodic()
    if any(local[a] and not runner._fused[a] for a in range(runner.dim)):
        # periodic images made by the ghost-layer kernels live in the arrays, not in the face buffers
        return False
    ref = runner._all_specs[0]
    for spec in runner._all_specs:
        if tuple(spec.location[1:]) != tuple(ref.location[1:]) or tuple(spec.size[1:]) != tuple(ref.size[1:]):
            return False        # faces that only partly overlap: rows of the two sides do not line up
        faces = set(face for face, _ in spec.connecting_subdomains())
        if not faces or not faces <= set((spec.X_LOW, spec.X_HIGH)):
            return False
        if spec.size[0] > 1024 or spec.size[0] < 2:
            return False
    return True


class Halo(object):
    """No neighbours: nothing crosses.  The surface the schemes share."""
    xface = nnx = chunks = None       # the dense face buffers / planes of the two x-slab schemes, the z-chunks of the first
    routes = ()                       # FaceBufferHalo: (neighbour id, my face) in the order pieces are posted
    shareable = False                 # buffers that neighbours of one process on one device can share

    def __init__(self, runner=None):
        self.runner = runner
        self.links, self.macro_links = {}, {}

    def of_kind(self, kind):
        return self.links if kind == 'dist' else self.macro_links

    def messages(self, kind, par):
        """[(neighbour id, send buffer, #send, receive buffer, #recv)] of the exchange `kind` of a step of parity `par`,
        ordered by neighbour id."""
        links = self.of_kind(kind)
        return [(nid, links[nid].send_bufs[par], links[nid].n_send, links[nid].recv_bufs[par], links[nid].n_recv)
                for nid in sorted(links)]

    def reset(self):
        """The state was just written from the host (initial conditions, a checkpoint, a debug write): the arrays count,
        nothing that crossed the faces before does."""

    def materialise(self):
        """Before anything reads the arrays on the host: what was received outside them goes into them."""

    def unbind(self):
        """A step program has set the module's face buffers itself."""


class IndexListHalo(Halo):
    """Index lists, device buffers and pack / unpack kernels for every neighbour.  A model with several lattices (binary
    fluids) sends them back to back in one message per neighbour; the non-local models also exchange the macroscopic
    fields their force reads at neighbouring nodes (reference _init_interblock_kernels / _send_macro / _recv_macro,
    subdomain_runner.py:1907-2100)."""

    def __init__(self, runner):
        Halo.__init__(self, runner)
        r = runner
        arr = list(reversed(r._physical_size))
        dense_nodes = r._get_nodes()
        links = subdomain_connection.build_halo_links(r._spec, r._all_specs, r._global_size, r._global_periodic,
                                                      r._sim.grid, arr, dense_nodes if r.indirect else r._dist_stride,
                                                      fused=r._fused)
        if r.indirect:
            r._translate_halo_links(links, r._host_indirect_address, dense_nodes, r._dist_stride)
        n_grids = len(r._gpu_grids_primary)
        for nid, link in list(links.items()):
            link.n_send = max(len(link.push_send), len(link.pull_send)) * n_grids
            link.n_recv = max(len(link.push_recv), len(link.pull_recv)) * n_grids
            if link.n_send == 0 and link.n_recv == 0:
                del links[nid]
        allocate(r._connector, r, 'dist', links, separate=False)
        for nid in sorted(links):
            self._population_kernels(links[nid])
        self.links = links
        if r.has_macro_exchange:
            self._init_macro(arr)

    def _population_kernels(self, link):
        """packs / unpacks [parity of the step they serve]: in place the even steps pull and the odd ones push, two-copy
        every step pushes and the steps of parity p write copy 1 - p."""
        r = self.runner
        b, n_grids, isz = r.backend, len(r._gpu_grids_primary), np.dtype(r.float).itemsize
        aa = r.config.access_pattern == 'AA'
        lists = {}
        for par, mode, copy in ((1, 'push', 0), (0, 'pull', 0)) if aa else ((1, 'push', 0), (0, 'push', 1)):
            if mode not in lists:
                s_idx, r_idx = getattr(link, mode + '_send'), getattr(link, mode + '_recv')
                lists[mode] = (s_idx, r_idx, b.alloc_buf(like=s_idx) if len(s_idx) else 0,
                               b.alloc_buf(like=r_idx) if len(r_idx) else 0)
            s_idx, r_idx, g_s, g_r = lists[mode]
            for g in range(n_grids):
                dist = r.gpu_dist(g, copy)
                if len(s_idx):
                    link.packs[par].append(r.get_kernel('CollectSparseData', [
                        g_s, dist, link.send_bufs[par] + g * len(s_idx) * isz, len(s_idx)], 'PPPi'))
                if len(r_idx):
                    link.unpacks[par].append(r.get_kernel('DistributeSparseData', [
                        g_r, dist, link.recv_bufs[par] + g * len(r_idx) * isz, len(r_idx)], 'PPPi'))

    def _init_macro(self, arr):
        r = self.runner
        cfg, dim = r.config, r.dim

        def fused_of(spec):
            return [int(bool(spec._periodicity[a]) and getattr(cfg, 'hip_fused_periodic', True)) for a in range(dim)]

        links = subdomain_connection.build_macro_links(r._spec, r._all_specs, r._global_size, r._global_periodic, arr,
                                                       fused_of)
        b = r.backend
        fields = [r.gpu_field(fp.buffer) for fp in r._sim._scalar_fields if fp.abstract.need_nn]
        isz = np.dtype(r.float).itemsize
        for nid, link in list(links.items()):
            link.n_send, link.n_recv = len(link.send) * len(fields), len(link.recv) * len(fields)
            if link.n_send == 0 and link.n_recv == 0:
                del links[nid]
        allocate(r._connector, r, 'macro', links, separate=False)
        for nid in sorted(links):
            link = links[nid]
            ns, nr = len(link.send), len(link.recv)
            g_s = b.alloc_buf(like=link.send) if ns else 0
            g_r = b.alloc_buf(like=link.recv) if nr else 0
            link.packs = [[r.get_kernel('CollectSparseData', [g_s, f, link.send_bufs[par] + i * ns * isz, ns], 'PPPi')
                           for i, f in enumerate(fields)] if ns else [] for par in (0, 1)]
            link.unpacks = [[r.get_kernel('DistributeSparseData', [g_r, f, link.recv_bufs[par] + i * nr * isz, nr], 'PPPi')
                             for i, f in enumerate(fields)] if nr else [] for par in (0, 1)]
        self.macro_links = links


class _FaceHalo(Halo):
    """What the two x-slab schemes share: face links without pack / unpack kernels, buffers that the subdomains of one
    process can share (controller.LocalGroup._share_xface_buffers)."""
    shareable = True
    planes = None       # the xface.XFaceHalo / xface.NNPlanes the sweeps are bound to; .shared: buffers not copied

    def adopt(self, kind, nid, bufs):
        """My send buffers towards `nid` become `bufs`: that neighbour's receive buffers (its memory and content stay:
        they may have been primed from a restored state)."""
        self.of_kind(kind)[nid].send_bufs = list(bufs)
        self.place()
        self.planes.shared = True


class FaceBufferHalo(_FaceHalo):
    """Per neighbour and step parity one send and one receive buffer (face_layout).  The sweep is cut into z-chunks and the
    planes a chunk completes travel at once (xface.ChunkPlan)."""

    @staticmethod
    def applies(runner):
        """Every subdomain of the simulation is connected through its x faces only, and the model can use the x-face
        buffers (same answer in every runner of the simulation)."""
        r = runner
        if not getattr(r.config, 'hip_xface', True) or r.has_macro_exchange or r.dim != 3 or \
                not getattr(r.backend, 'supports_xface', False):
            return False
        if not xface.supported(r._sim.grid, r._desc, r.indirect) or len(r._sim.grids) != 1:
            return False
        return x_slabs_line_up(r)

    def __init__(self, runner):
        Halo.__init__(self, runner)
        r = runner
        self.count = xface.face_count(r._desc)
        self.links = face_links(r._spec, self.count)
        zc = getattr(r._connector, 'zero_copy', False)
        allocate(r._connector, r, 'dist', self.links, separate=True)
        # pieces are posted in this order on both sides: my low <-> its high first
        self.routes = [(nid, face) for nid in sorted(self.links) for face in self.links[nid].faces]
        send, recv = self._tables()
        self.xface = self.planes = xface.XFaceHalo(r.backend, r.module, r._sim.grid, r._desc, send, recv, shared=zc)
        lat = list(reversed(r._lat_size))
        # several launches per step pay off where the transfer is slow (another process / GPU: a connector that can be
        # called in the middle of a step); runners stepped in lock-step by one Python process are bound by that process
        # instead: one chunk (profiles/r03/xface_overlap_schemes.jsonl)
        self.chunks = xface.ChunkPlan(lat[2] - 2, r._fused[2], None if getattr(r._connector, 'mid_step', False) else 1)

    def _tables(self):
        send, recv = [[0, 0], [0, 0]], [[0, 0], [0, 0]]
        isz = np.dtype(self.runner.float).itemsize
        for link in self.links.values():
            for par, face, s, rcv in face_layout(link, self.count, isz):
                send[par][face], recv[par][face] = s, rcv
        return send, recv

    def place(self):
        """The face addresses inside the links' buffers (again after a buffer of a link was replaced)."""
        self.xface.send, self.xface.recv = self._tables()
        self.xface._bound = None

    def unbind(self):
        self.xface._bound = None

    def pieces(self, pos, par, kind):
        """[(neighbour id, send address, receive address, elements)] of batch `pos` of a step of parity `par` and chunk
        kind `kind`: for every connected face (send side: my faces low, high; the receive side of the same neighbour takes
        them as its high, low) the runs of z-planes the chunks swept so far have completed."""
        x, isz = self.xface, np.dtype(self.runner.float).itemsize
        out = []
        # sends in my face order; receives of one neighbour in the order IT sends: its low face (= my high) first
        for nid in sorted(self.links):
            s_faces = self.links[nid].faces
            for sf, rf in zip(s_faces, reversed(s_faces)):
                for p0, p1 in self.chunks.batches[kind][pos]:
                    off, cnt = p0 * x.plane * isz, (p1 - p0) * x.plane
                    out.append((nid, x.send[par][sf] + off, x.recv[par][rf] + off, cnt))
        return out

    def reset(self):
        r = self.runner
        r.backend.sync_stream(*r._all_streams())
        r._connector.quiesce(r)       # peer transport: the neighbours write into these buffers themselves
        self.xface.reset(r._calc_stream)
        it = r._sim.iteration
        if r.config.access_pattern == 'AA' and (it & 1):
            # the next step pulls, and the edge lanes of the fluid-only row kernel take what enters through a
            # connected x face from the receive buffers alone (slf_row.hip: no pull out of the ghost column): prime
            # them from the ghost columns of the state just written (a checkpoint taken at an odd iteration)
            self.xface.prime_pull(r.gpu_dist(0, 0), r._calc_stream, parity=1 - (it & 1))
        r.backend.sync_stream(r._calc_stream)
        r._connector.quiesce(r)
        r._step_parity = None

    def materialise(self):
        """The arrays are stale at the connected faces until the received values are written into them."""
        r = self.runner
        if r._step_parity is None:
            return
        r.backend.sync_stream(*r._all_streams())
        self.xface.materialise(r.gpu_dist(0, r._step_copy), not r._step_pulls, r._calc_stream, parity=r._step_parity)
        r.backend.sync_stream(r._calc_stream)


class PlaneHalo(_FaceHalo):
    """Per neighbour, kind ('dist': every lattice, 'macro': rho and phi) and step parity one send and one receive buffer,
    laid out as in FaceBufferHalo.  The links carry no pack / unpack kernels -- the sweeps fill and read the planes -- so
    the step program of the general case (pack -> exchange -> unpack, per kind) moves them as it stands."""

    @staticmethod
    def applies(runner):
        r = runner
        if not r.has_macro_exchange or not getattr(r.config, 'hip_xface', True) or r.dim != 3 or \
                len(r._sim.grids) not in (1, 2) or not getattr(r.backend, 'supports_xface_planes', False):
            return False
        if not xface.supported_nn(r._sim.grid, r._desc, r.indirect):
            return False
        # (An edge node in a row next to a y / z face that is not wrapped inside the kernels reads ghost-row entries of the
        # density planes.  They hold what prime() found in the neighbour's ghost row -- the +inf every field is created
        # with outside the lattice, make_scalar_field -- which is what the ghost COLUMN of such a row holds as well: no
        # node owns that position, so build_macro_links never delivers anything there.  A node that computes a force must
        # not sit there in either scheme; a wall does not care.)
        return x_slabs_line_up(r)

    def __init__(self, runner):
        Halo.__init__(self, runner)
        r = runner
        self.nnx = self.planes = xface.NNPlanes(r.backend, r.module, r._sim.grid, r._desc, n_lat=len(r._sim.grids))
        for kind in ('dist', 'macro'):
            links = face_links(r._spec, self.nnx.count[kind])
            allocate(r._connector, r, kind, links, separate=True)
            self.of_kind(kind).update(links)
        zc = getattr(r._connector, 'zero_copy', False)
        self.nnx.shared = bool(zc)
        r.config.logger.debug('subdomain %d: Shan-Chen model over x-face planes (%s)' % (
            r._spec.id, 'the neighbours\' memory mapped here' if zc else type(r._connector).__name__))
        self.place()
        self.nnx.reset()

    def place(self):
        """The face addresses inside the links' buffers (again after a buffer of a link was replaced)."""
        nnx = self.nnx
        for kind in ('dist', 'macro'):
            for link in self.of_kind(kind).values():
                for par, face, s, rcv in face_layout(link, nnx.count[kind], nnx.isz):
                    nnx.send[kind][par][face], nnx.recv[kind][par][face] = s, rcv

    def reset(self):
        r = self.runner
        r.backend.sync_stream(*r._all_streams())
        r._connector.quiesce(r)       # zero-copy transports: the neighbours write into these planes themselves
        self.nnx.reset(r._calc_stream)
        r.backend.sync_stream(r._calc_stream)
        r._connector.quiesce(r)       # ... and I into theirs: everybody has cleared before anybody fills
        self.prime()
        group = getattr(r, '_group', None)
        if group is not None and self.nnx.shared:
            # subdomains of one process reset one at a time: what the neighbours had filled in my planes went with the
            # clearing above
            for other in group.runners:
                if other is not r and other._nnx is not None:
                    other._halo.prime()
        r._connector.quiesce(r)
        r._step_parity = None

    def prime(self):
        """The density planes I send, from the fields as they are on the device now (xface.NNPlanes.prime)."""
        r = self.runner
        fields = [r.gpu_field(fp.buffer) for fp in r._sim._scalar_fields if fp.abstract.need_nn]
        self.nnx.prime(fields, r._calc_stream)
        if r.config.access_pattern == 'AA':
            self.nnx.prime_own([r.gpu_dist(g, 0) for g in range(self.nnx.n_lat)], r._calc_stream)
        r.backend.sync_stream(r._calc_stream)

    def materialise(self):
        r = self.runner
        if r._step_parity is None:
            return
        r.backend.sync_stream(*r._all_streams())
        self.nnx.materialise([r.gpu_dist(g, r._step_copy) for g in range(self.nnx.n_lat)], not r._step_pulls,
                             r._calc_stream, r._step_parity)
        r.backend.sync_stream(r._calc_stream)


def make(runner):
    """The halo scheme of `runner` (every runner of a simulation picks the same one)."""
    if runner._all_specs is None or len(runner._all_specs) < 2:
        return Halo(runner)
    if runner._connector is None:
        from sailfish_amd.connector import LocalConnector
        runner._connector = LocalConnector()
    for scheme in (PlaneHalo, FaceBufferHalo):
        if scheme.applies(runner):
            return scheme(runner)
    return IndexListHalo(runner)
