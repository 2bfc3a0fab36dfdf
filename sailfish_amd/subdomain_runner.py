"""Per-subdomain driver: memory, kernels, the time-step loop, halo exchange,
output and checkpoints (reference sailfish/subdomain_runner.py).

One runner = one subdomain on one GPU.  The step keeps the reference's structure
(subdomain_runner.py:960-1139):

    calc stream: [wait for the previous halo]  sweep(boundary regions) -> event -> sweep(bulk)
                 -> periodic-boundary kernels of locally periodic axes
    halo stream: wait(event) -> pack (index-list gather) -> exchange -> unpack -> event

but everything stays on the device: the pack kernels write straight into the
send buffer, buffers travel GPU-to-GPU (RCCL over xGMI through torch.distributed,
or a peer copy when both subdomains live in this process), the unpack kernels
scatter into the neighbour-owned slots.  The reference stages every halo through
pinned host memory and a zmq socket (subdomain_runner.py:1064-1139).

Launch geometry is a region of rows / planes (`backend.run_kernel(kernel, region)`)
instead of the reference's bulk / boundary block arithmetic (:396-475).
"""
import math
import os
import pickle
import time
import weakref

import numpy as np

from sailfish_amd import halo, hipabi, io, subdomain_connection, util, xface
from sailfish_amd import node_type as nt
from sailfish_amd.lb_base import LBMixIn, LBSim
from sailfish_amd.profile import TimeProfile
from sailfish_amd.stepqueue import DirectQueue, StepPlans


class GPUBuffer(object):
    """Host/device buffer pair (reference subdomain_runner.py:29-42)."""

    def __init__(self, host_buffer, backend):
        self.host = host_buffer
        self.gpu = backend.alloc_buf(like=host_buffer) if host_buffer is not None else None


_hup_runners = weakref.WeakSet()        # runners that take part in SIGHUP -> checkpoint (_install_signal_handlers)
_hup_state = {'previous': None}         # what handled SIGHUP before the first runner of the process


def _hup_dispatch(signum, frame):
    for runner in list(_hup_runners):
        runner.sighup_handler(signum, frame)
    if callable(_hup_state['previous']):
        _hup_state['previous'](signum, frame)


class SubdomainRunner(object):
    """Runs the simulation for a single SubdomainSpec."""

    def __init__(self, simulation, spec, output, backend, quit_event=None, summary_addr=None, master_addr=None,
                 summary_channel=None):
        self._sim = simulation
        self._spec = spec
        self._output = output
        self.backend = backend
        if quit_event is None:          # always there: a user hook ends the run with runner._quit_event.set()
            import threading
            quit_event = threading.Event()
        self._quit_event = quit_event
        self.config = simulation.config
        self._spec.runner = self
        self._bcg = None
        self._scalar_fields = []
        self._vector_fields = []
        self._gpu_field_map = {}
        self._host_base = {}
        self._gpu_grids_primary = []
        self._gpu_grids_secondary = []
        self._kernels_prepared = False
        self._halo = halo.Halo()
        self._connector = None
        self._all_specs = None
        self._global_size = None
        self._global_periodic = None
        self.timing = {'steps': 0, 'wall': 0.0}
        self._profile = TimeProfile(self)
        self._checkpoint_req = False      # set by SIGHUP (reference sighup_handler, :1528-1535)
        self._init_geometry_done = False
        if not hasattr(self.config, 'logger'):
            self.config.logger = util.setup_logger(self.config)

    # ------------------------------------------------------------------ geometry
    @property
    def dim(self):
        return self._spec.dim

    def set_topology(self, all_specs, global_size, periodic):
        """all_specs: every SubdomainSpec of the simulation (for halo routing)."""
        self._all_specs = all_specs
        self._global_size = list(global_size)
        self._global_periodic = list(periodic)

    def ghost_owner_map(self, spec):
        if self._all_specs is None or len(self._all_specs) < 2:
            return np.zeros(list(reversed(spec.actual_size)), dtype=bool)
        return subdomain_connection.ghost_owned_by_others(spec, self._all_specs, self._global_size,
                                                          self._global_periodic)

    def _init_shape(self):
        """Logical (ghost-including) and physical (x padded) sizes, reference subdomain_runner.py:359-373."""
        self._lat_size = list(reversed(self._spec.actual_size))
        self._physical_size = list(reversed(self._spec.actual_size))
        alignment = self.config.mem_alignment
        self._physical_size[-1] = int(math.ceil(float(self._physical_size[-1]) / alignment)) * alignment
        if self._global_size is None:
            gs = [self.config.lat_nx, self.config.lat_ny] + ([self.config.lat_nz] if self.dim == 3 else [])
            per = [self.config.periodic_x, self.config.periodic_y] + \
                ([self.config.periodic_z] if self.dim == 3 else [])
            self.set_topology([self._spec], gs, per)
        self._global_shape = tuple(reversed(self._global_size))

    def _get_nodes(self):
        return int(np.prod(self._physical_size))

    @property
    def num_phys_nodes(self):
        return self._get_nodes()

    @property
    def float(self):
        return np.float32 if self.config.precision == 'single' else np.float64

    def _lat_view(self, buf):
        sl = tuple(slice(0, n) for n in self._lat_size)
        return buf[sl]

    def make_scalar_field(self, dtype=None, name=None, register=True, async_=False, gpu_array=False,
                          nonghost_view=True):
        """Allocates a host array of the padded size and returns a view of the lattice (ghost nodes
        excluded unless nonghost_view=False).  Float fields are filled with +inf in the ghost layer and 0
        elsewhere (reference subdomain_runner.py:253-320)."""
        if dtype is None:
            dtype = self.float
        size = self._get_nodes()
        if async_:
            buf = self.backend.alloc_async_host_buf(size, dtype)
        else:
            buf = np.zeros(size, dtype=dtype)
        buf = buf.reshape(self._physical_size)
        if np.issubdtype(dtype, np.floating):
            buf[:] = np.inf
        fview = self._lat_view(buf)
        self._host_base[id(fview)] = buf
        if nonghost_view:
            view = fview[self._spec._nonghost_slice]
            if np.issubdtype(dtype, np.floating):
                view[:] = 0.0
            self._host_base[id(view)] = buf
        else:
            view = fview
        self._lat_views = getattr(self, '_lat_views', {})
        self._lat_views[id(view)] = buf
        if register:
            self._scalar_fields.append(view)
            if name is not None and self._output is not None:
                self._output.register_field(view, name)
        return view, None

    def make_vector_field(self, name=None, output=False, async_=False, gpu_array=False):
        components = [self.make_scalar_field(self.float, register=False, async_=async_)[0]
                      for _ in range(self.dim)]
        self._vector_fields.append(components)
        if name is not None and self._output is not None:
            self._output.register_field(components, name)
        return components

    def field_base(self, field):
        """The whole padded host array (ghosts + x padding) behind a field returned by make_scalar_field."""
        return self._lat_views[id(field)]

    def visualization_map(self):
        return self._subdomain.visualization_map()

    def _init_geometry(self):
        self._init_shape()
        self._subdomain = self._sim.subdomain(self._global_shape, self._spec, self._sim.grid)
        self._subdomain.allocate()
        self._subdomain.reset()
        self._init_geometry_done = True

    # ------------------------------------------------------------------ compute setup
    def _local_periodic(self):
        return [bool(self._spec._periodicity[a]) for a in range(self.dim)]

    def _module_desc(self):
        cfg = self.config
        lat = list(reversed(self._lat_size))
        arr = list(reversed(self._physical_size))
        kw = dict(precision=4 if cfg.precision == 'single' else 8,
                  access_pattern=hipabi.SLF_AA if cfg.access_pattern == 'AA' else hipabi.SLF_AB,
                  lat_nx=lat[0], lat_ny=lat[1], lat_nz=lat[2] if self.dim == 3 else 1,
                  arr_nx=arr[0], arr_ny=arr[1], arr_nz=arr[2] if self.dim == 3 else 1)
        self._sim.fill_module_desc(kw)
        kw.update(self._subdomain._encoder.desc_fields())
        if hasattr(self._sim, 'check_module_desc'):
            self._sim.check_module_desc(kw)
        local = self._local_periodic()
        fused = [int(local[a] and getattr(cfg, 'hip_fused_periodic', True)) for a in range(self.dim)]
        kw['periodic_local'] = [int(x) for x in local] + [0] * (3 - self.dim)
        kw['periodic_fused'] = fused + [0] * (3 - self.dim)
        self._fused = fused
        if hasattr(self._sim, 'fill_subdomain_desc'):       # what depends on this subdomain's faces and node map
            self._sim.fill_subdomain_desc(self, kw)
        # fast path: every real node is a plain fluid node -> the sweep does not read the node map (ghost
        # nodes behind an unconnected, non-periodic face are never pulled from by a fluid-only interior
        # in any way that matters: what they hold is what a wall of excluded nodes would hold)
        vis = self._subdomain.visualization_map()
        kw['fluid_only'] = int(np.all(vis == 0))
        excluded = np.isin(vis, [nt._NTUnused.id, nt._NTGhost.id, nt._NTPropagationOnly.id])
        kw['sparse_geometry'] = int(excluded.mean() > 0.05)
        if self.indirect:
            # distributions hold the active nodes only; everything else stays dense
            if any(local[a] and not fused[a] for a in range(self.dim)):
                raise ValueError('--node_addressing=indirect needs in-sweep periodic boundaries '
                                 '(do not combine with --nohip_fused_periodic)')
            kw['fluid_only'] = 0
            kw['node_addressing'] = hipabi.SLF_ADDR_INDIRECT
            if hasattr(self._sim, 'check_lattice'):
                self._sim.check_lattice(kw)
            if hasattr(self._sim, 'check_accel_field'):
                self._sim.check_accel_field(kw)
            kw['dist_stride'] = (self._subdomain.active_nodes + 1 + 31) // 32 * 32   # + one spare slot (halo lists)
            self._check_halfbb_targets()
        return hipabi.make_desc(**kw)

    def _check_halfbb_targets(self):
        """Indirect addressing, in-place pattern: a half-way bounce-back node is a wet node whose even step stores the
        population it reflects into the slot of the node behind the wall (slf_sweep.h; reference boundary.mako:653-683 with
        propagation.mako:93-99).  A node without a slot cannot take it: the sweep would drop the store and the run would go on
        with a population missing on every such link -- finite, and another flow.  (The reference indexes nodes[] unguarded
        there.)  Refused here, before anything is built or launched."""
        if self.config.access_pattern != 'AA':
            return                                  # the two-copy step stores into the node's own slot
        sub = self._subdomain
        # (Tamm-Mott-Smith walls end their step with the same store)
        pos = np.argwhere(np.isin(sub.visualization_map(), (nt.NTHalfBBWall.id, nt.NTWallTMS.id)))    # real nodes, numpy axis order
        if not len(pos):
            return
        grid = self._sim.grid
        codes = sub._orientation[tuple(pos.T)].astype(np.int64)                 # link tags, or an orientation code
        tagged = bool(getattr(self.config, 'use_link_tags', True))
        mask = sub.active_node_mask
        shape = np.array(sub.lat_shape)
        wrap = list(reversed(self._local_periodic()))
        es = self._spec.envelope_size
        lost = np.zeros(len(pos), dtype=np.int64)
        for bit, vec in enumerate(grid.basis[1:]):
            if tagged:
                missing = ((codes >> bit) & 1) == 0                             # the direction points to a non-fluid node
            else:
                normal = np.array([grid.dir_to_vec(int(c)) if c else [0] * self.dim for c in codes])
                missing = (normal * np.array([int(c) for c in vec])).sum(axis=1) < 0
            target = pos + np.array([int(c) for c in reversed(vec)])
            for axis in range(self.dim):
                if wrap[axis]:
                    target[:, axis] %= shape[axis]
            lost += missing & ~mask[tuple((target + es).T)]
        if lost.any():
            first = pos[np.nonzero(lost)[0][0]]
            where = tuple(int(c) + int(o) for c, o in zip(reversed(first), self._spec.location))
            raise ValueError('--node_addressing=indirect with --access_pattern=AA: %d links of half-way bounce-back / TMS nodes point '
                             'to nodes that own no slot in the distribution arrays (first at node %s): the populations '
                             'reflected there would be lost.  Keep the layer behind half-way bounce-back walls in the '
                             'active-node map (count those wall nodes as fluid in the wall map given to '
                             'set_active_node_map_from_wall_map), or use full-way bounce-back walls or the two-copy '
                             'pattern (--access_pattern=AB).' % (int(lost.sum()), where))

    @property
    def indirect(self):
        return getattr(self.config, 'node_addressing', 'direct') == 'indirect'

    def _indirect_address_host(self):
        """Dense table node -> slot (or SLF_INVALID_NODE) over the padded arrays, slots numbered in memory
        order of the active nodes so that neighbouring active nodes have neighbouring slots
        (reference _build_indirect_address_map, :829-837)."""
        addr, _ = self.make_scalar_field(np.uint32, register=False, nonghost_view=False)
        base = self._host_base[id(addr)]
        base[:] = hipabi.SLF_INVALID_NODE
        mask = self._subdomain.active_node_mask
        addr[mask] = np.arange(int(mask.sum()), dtype=np.uint32)
        return base

    def _build_indirect_address_map(self):
        self._host_indirect_address = self._indirect_address_host()
        self._gpu_indirect_address = self.backend.alloc_buf(like=self._host_indirect_address)

    def _translate_halo_links(self, links, addr_base, dense_nodes, dist_stride):
        """Halo index lists (population * dense_nodes + dense node) -> (population * dist_stride + slot).
        Halo nodes next to solid regions own no slot: they are routed to the spare slot behind the last
        active node, so that both sides of a link keep lists of the same length and order."""
        addr = addr_base.reshape(-1).astype(np.uint64)
        spare = np.uint64(self._subdomain.active_nodes)
        for link in links.values():
            for kind in ('push_send', 'push_recv', 'pull_send', 'pull_recv'):
                idx = getattr(link, kind)
                q, node = idx // np.uint64(dense_nodes), idx % np.uint64(dense_nodes)
                slot = addr[node.astype(np.int64)]
                slot[slot == np.uint64(hipabi.SLF_INVALID_NODE)] = spare
                setattr(link, kind, np.ascontiguousarray(q * np.uint64(dist_stride) + slot, dtype=np.uint64))
        return links

    def gpu_indirect_address(self):
        return self._gpu_indirect_address

    def add_indirect_args(self, args, signature):
        """Indirect modules take the address table as an additional first kernel argument
        (reference _add_indirect_args, :1153-1157)."""
        if self.indirect:
            return [self.gpu_indirect_address()] + list(args), 'P' + signature
        return list(args), signature

    def _init_compute(self):
        self._desc = self._module_desc()
        self.module = self.backend.build(self._desc)
        spec = self._spec
        if hasattr(self.backend, 'set_x_ghost_unused') and not self._local_periodic()[0] and \
                not getattr(self.config, 'debug_dump_dists', False) and os.environ.get('SLF_X_GHOST_STORES', '0') != '1':
            # ghost columns behind an x face that is neither periodic nor connected.  Two-copy pattern: nothing ever
            # reads them.  In-place pattern: the odd step of the first / last real column PULLS out of them what its even
            # step pushed there two steps earlier (the reference's behaviour for a wet node next to an open face), so the
            # stores may only go where that column holds no wet node -- a wall, as in every cavity / channel / pipe: what
            # a dry node pulls out of the ghost column only ever travels back into it.  (Raw dumps of the arrays keep the
            # reference's pushes: --debug_dump_dists.)
            wet = self._subdomain.fluid_map(wet=True)
            ab = self.config.access_pattern == 'AB'
            low = not spec.has_face_conn(spec.X_LOW) and (ab or not wet[..., 0].any())
            high = not spec.has_face_conn(spec.X_HIGH) and (ab or not wet[..., -1].any())
            self.backend.set_x_ghost_unused(self.module, low, high)
        self._calc_stream = self.backend.make_stream()
        # the halo stream: ahead of the bulk sweep's queued workgroups where the backend can say so
        # (not with the peer transport: its waits are kernels that spin on this stream until the neighbours have signalled,
        # and a spinning kernel in a high-priority queue holds the sweeps back -- DESIGN.md §7)
        prio = getattr(self.backend, 'supports_stream_priority', False) and os.environ.get('SLF_HALO_PRIORITY', '1') != '0' and \
            not getattr(self._connector, 'zero_copy', False)
        self._data_stream = self.backend.make_stream(high_priority=True) if prio else self.backend.make_stream()
        self._dist_stride = hipabi.dist_stride(self._desc)

    def _init_gpu_data(self):
        self._alloc_distributions()     # first: placed arrays want an allocator that has handed out nothing yet
        b = self.backend
        # fields and node map: x = 1 of every row on a 128-byte line, like the distributions (the sweeps read / store them
        # with the lane offsets of the populations: aligned accesses, 8-byte ones in the two-nodes-per-thread kernels)
        def aligned(host):
            kw = {'align_offset': b.dist_align_offset(host.dtype.itemsize)} if hasattr(b, 'dist_align_offset') else {}
            return b.alloc_buf(like=host, **kw)
        for field in self._scalar_fields:
            self._gpu_field_map[id(field)] = aligned(self._host_base[id(field)])
        for vec in self._vector_fields:
            for comp in vec:
                self._gpu_field_map[id(comp)] = aligned(self._host_base[id(comp)])
        self._gpu_geo_map = aligned(self._host_base[id(self._subdomain._type_map_ghost)])
        self.row_classes = None
        if getattr(b, 'supports_row_classes', None) and b.supports_row_classes(self._desc) and \
                getattr(self.config, 'hip_row_classes', True) and os.environ.get('SLF_ROW_CLASSES', '1') != '0':
            # which waves need the map at all, which rows need boundary-condition code (backend_hip.classify_rows)
            self.row_classes = b.classify_rows(self.module, self._gpu_geo_map, self._calc_stream)
            self.config.logger.debug('row classes: %s' % self.row_classes)
        if self.indirect:
            self._build_indirect_address_map()
        self._init_accel_field(aligned)

    def accel_field_host(self):
        """The acceleration field of this subdomain as the sweep reads it: [dim] + the padded array shape, in the run's
        precision -- the simulation's position-dependent body forces (LBForcedSim.accel_field_at) at the GLOBAL
        coordinates of the real nodes, evaluated in float64 and rounded once; ghost and padding nodes hold 0."""
        field = np.zeros((self.dim,) + tuple(self._physical_size), dtype=self.float)
        grids = self._subdomain._get_mgrid()                     # global (hx, hy[, hz]) of the real nodes
        vals = self._sim.accel_field_at(tuple(np.asarray(g, dtype=np.float64).ravel() for g in grids))
        real = self._spec._nonghost_slice
        for d in range(self.dim):
            self._lat_view(field[d])[real] = vals[d].reshape(grids[0].shape)
        return field

    def _init_accel_field(self, alloc):
        """A body force that depends on position: evaluated once, uploaded once, handed to the module.  The field is not
        state: every prepare() -- a restored run included -- evaluates it again."""
        self._gpu_accel_field = None
        if not getattr(self._sim, 'has_accel_field', False):
            return
        self._host_accel_field = self.accel_field_host()
        self._gpu_accel_field = alloc(self._host_accel_field)
        self.backend.set_accel_field(self.module, self._gpu_accel_field)

    def _alloc_distributions(self):
        b = self.backend
        nbytes = self._sim.grid.Q * self._dist_stride * self.float().itemsize
        off = b.dist_align_offset(self.float().itemsize)
        ab = self.config.access_pattern == 'AB'
        from sailfish_amd import placement
        if placement.enabled() and nbytes >= placement.MIN_BYTES and not self.indirect and \
                getattr(self.config, 'hip_placement', True):
            # large arrays: physical backing spread over HBM (placement.py); all lattices and copies share the span
            n = len(self._sim.grids)
            sizes = [nbytes] * (n * (2 if ab else 1))
            cfg = self.config
            if getattr(cfg, 'hip_placement_tune', True) and os.environ.get('SLF_PLACEMENT_TUNE', '1') != '0' and \
                    not (0 < cfg.max_iters < 200) and not placement.holding_now():
                # placement by measurement: a second set is placed while the first is allocated, the faster one stays
                bufs, self.placement_tuning = placement.choose(
                    lambda: b.alloc_placed(sizes, off), lambda bs: self._probe_placement(bs, n, ab),
                    lambda bs: [b.free_buf(pb.addr) for pb in bs], log=cfg.logger.debug,
                    room=lambda: placement.room_for(b, sum(sizes)))
            else:
                bufs = b.alloc_placed(sizes, off)
            self._gpu_grids_primary = [pb.addr for pb in bufs[:n]]
            self._gpu_grids_secondary = [pb.addr for pb in bufs[n:]]
            self.config.logger.debug('placed distributions: %s' % b.last_placement)
        else:
            for _ in self._sim.grids:
                self._gpu_grids_primary.append(b.alloc_buf(size=nbytes, align_offset=off))
                if ab:
                    self._gpu_grids_secondary.append(b.alloc_buf(size=nbytes, align_offset=off))
        if self.indirect:
            # the spare slot the halo lists route slot-less nodes to (and the padding behind it) is written by no sweep: it
            # starts as the "never written" sentinel the halo kernels do not deliver, like the ghost slots of dense arrays
            # (whose fields start from +inf) -- a zero would travel into the slot of a wall node across the seam
            fill = np.zeros((self._sim.grid.Q, self._dist_stride), dtype=self.float)
            fill[:, self._subdomain.active_nodes:] = np.nan
            for addr in self._gpu_grids_primary + self._gpu_grids_secondary:
                b.to_buf(addr, fill)
        self.config.logger.debug('distributions: %d MiB' % (nbytes * (2 if self._gpu_grids_secondary else 1) >> 20))

    placement_tuning = None

    def _probe_placement(self, bufs, n_grids, ab, steps=12):
        """Seconds per step of the plain fluid sweep on the first lattice of the placed set `bufs`: what
        placement.choose() compares (placement.probe_sweep)."""
        from sailfish_amd import placement
        nbytes = self._sim.grid.Q * self._dist_stride * self.float().itemsize
        src, dst = bufs[0].addr, (bufs[n_grids].addr if ab else bufs[0].addr)
        return placement.probe_sweep(self.backend, self._desc, self.dim, src, dst, nbytes, self._calc_stream, steps)

    def gpu_field(self, field):
        if isinstance(field, list):
            return [self._gpu_field_map[id(f)] for f in field]
        return self._gpu_field_map[id(field)]

    def gpu_dist(self, num, copy):
        """Device address of lattice `num`, copy 0 (A) or 1 (B; the same buffer as A in the AA pattern)."""
        if copy == 0:
            return self._gpu_grids_primary[num]
        if self._gpu_grids_secondary:
            return self._gpu_grids_secondary[num]
        return self._gpu_grids_primary[num]

    def gpu_geo_map(self):
        return self._gpu_geo_map

    @property
    def gpu_scratch_space(self):
        return None

    def get_kernel(self, name, args, args_format, block_size=None, needs_iteration=False, shared=0,
                   more_shared=False):
        return self.backend.get_kernel(self.module, name, block=block_size or (self.config.block_size,),
                                       args=[int(a) for a in args], args_format=args_format, shared=shared,
                                       needs_iteration=needs_iteration)

    def exec_kernel(self, name, args, args_format, needs_iteration=False):
        kernel = self.get_kernel(name, args, args_format, needs_iteration=needs_iteration)
        self.backend.run_kernel(kernel, None, self._calc_stream)

    # ------------------------------------------------------------------ halo (sailfish_amd/halo.py)
    def _init_halo(self):
        """The halo scheme of this subdomain: links, device buffers, pack / unpack kernels or face buffers."""
        self._halo = halo.make(self)

    _links = property(lambda self: self._halo.links)                  # populations: {neighbour id: Link}
    _macro_links = property(lambda self: self._halo.macro_links)      # fields of the non-local models
    _xface = property(lambda self: self._halo.xface)                  # xface.XFaceHalo of a FaceBufferHalo, else None
    _nnx = property(lambda self: self._halo.nnx)                      # xface.NNPlanes of a PlaneHalo, else None
    _xface_routes = property(lambda self: self._halo.routes)
    _xchunks = property(lambda self: self._halo.chunks)

    def xface_pieces(self, pos):
        """The transfers of batch `pos` of the step just enqueued (halo.FaceBufferHalo.pieces)."""
        return self._halo.pieces(pos, self._step_parity, self._xface_kind)

    def halo_messages(self, kind='dist'):
        """[(neighbour id, send buffer, #send, receive buffer, #recv)] of the exchange that is due now,
        ordered by neighbour id: 'dist' = populations of the step just computed, 'macro' = fields read
        by non-local models."""
        return self._halo.messages(kind, self._step_parity)

    # ------------------------------------------------------------------ kernels
    def _prepare_compute_kernels(self):
        self._kernels_full = self._sim.get_compute_kernels(self, True, True)
        self._kernels_none = self._sim.get_compute_kernels(self, False, True)
        self._pbc_kernels = self._sim.get_pbc_kernels(self)
        self._pbc_axes = [a for a in range(self.dim) if self._local_periodic()[a] and not self._fused[a]]
        self._regions = self._make_regions()
        self._kernels_prepared = True

    def _make_regions(self):
        """(boundary regions, bulk region): rows / planes next to faces that exchange halos are swept
        first so that packing and the transfer overlap the bulk sweep (reference subdomain_runner.py:
        1028-1058).  x faces cannot be split off (a workgroup owns whole rows)."""
        lat = list(reversed(self._lat_size))
        ny = lat[1] - 2
        nz = lat[2] - 2 if self.dim == 3 else 1
        y0, y1 = 1, ny + 1
        z0, z1 = (1, nz + 1) if self.dim == 3 else (0, 1)
        full = (y0, y1, z0, z1)
        spec = self._spec
        if not self._links or not getattr(self.config, 'bulk_boundary_split', True):
            return [], full
        if spec.has_face_conn(spec.X_LOW) or spec.has_face_conn(spec.X_HIGH):
            return [], full
        z_conn = self.dim == 3 and (spec.has_face_conn(spec.Z_LOW) or spec.has_face_conn(spec.Z_HIGH))
        y_conn = spec.has_face_conn(spec.Y_LOW) or spec.has_face_conn(spec.Y_HIGH)
        if (z_conn and nz <= 2) or (y_conn and ny <= 2):
            # a connected face whose layer cannot be split off: its ghosts would be written by the bulk launch,
            # after the event the pack waits for -- sweep everything first
            return [], full
        bnd = []
        bz0, bz1 = z0, z1
        if self.dim == 3:
            if spec.has_face_conn(spec.Z_LOW):
                bnd.append((y0, y1, 1, 2))
                bz0 = 2
            if spec.has_face_conn(spec.Z_HIGH):
                bnd.append((y0, y1, nz, nz + 1))
                bz1 = nz
        by0, by1 = y0, y1
        if spec.has_face_conn(spec.Y_LOW):
            bnd.append((1, 2, bz0, bz1))
            by0 = 2
        if spec.has_face_conn(spec.Y_HIGH):
            bnd.append((ny, ny + 1, bz0, bz1))
            by1 = ny
        if not bnd:
            return [], full
        return bnd, (by0, by1, bz0, bz1)

    # ------------------------------------------------------------------ stepping
    has_macro_exchange = False

    def step(self, sync_req=False):
        """One time step of a runner that owns its process (neighbours, if any, live in other processes): the step is
        ONE program (_program, stepqueue.py), replayed from a C-ABI step plan -- a single runtime call -- where the
        transport can be part of it (RCCL through the C ABI), performed entry by entry otherwise (torch.distributed) and
        on the steps that record timing events."""
        b = self.backend
        it = self._sim.iteration
        self._update_dynamic_params(it)
        self._set_step_state(it)
        self._step_plans.run((it & 1, bool(sync_req)), it, lambda q: self._program(q, it, sync_req), [b],
                             may_plan=not self._profile.wants_gpu_events())
        self._halo.unbind()         # (a plan sets the module's face buffers itself)
        self._sim.iteration += 1
        b.set_iteration(self._sim.iteration)

    def _time_dependent(self):
        enc = getattr(self._subdomain, '_encoder', None)
        return (enc is not None and getattr(enc, 'time_dependent', False)) or getattr(self._sim, 'time_dependent_force', False)

    def _update_dynamic_params(self, it):
        """Boundary values that depend on time (node_type.DynamicValue with sym.S.time / time series; reference: device
        code, boundary.mako:52-84): evaluated on the host for LB iteration `it` and written into the kernels' parameter
        table on the calc stream, in front of the step's launches (C ABI slf_module_update_node_params; a one-wave kernel
        whose arguments ARE the values: the host does not wait)."""
        if self._time_dependent():
            for first, values in self._subdomain._encoder.dynamic_updates(it):
                self.backend.update_node_params(self.module, first, values, self._calc_stream)
            if getattr(self._sim, 'time_dependent_force', False):
                # the acceleration is an argument of the sweep launches: the ones enqueued from here on take this value
                self.backend.set_body_force(self.module, self._sim.body_force_at(it))

    # ------------------------------------------------------------------ the step as a program (stepqueue.py)
    def _init_step_program(self):
        """Events, streams and plan table of step() (runners that own their process; a same-process group keeps the
        three-phase step_compute / exchange / step_finish protocol of controller.LocalGroup)."""
        b = self.backend
        self._step_plans = StepPlans(b, getattr(b, 'supports_step_plans', False) and getattr(self.config, 'hip_step_plans', True) and
                                     os.environ.get('SLF_STEP_PLAN', '1') != '0')
        names = ('bnd', 'bulk', 'halo', 'packed', 'copied', 'macro', 'macro_halo', 'macro_packed', 'macro_copied')
        self._pev = [dict((n, b.make_event(self._calc_stream)) for n in names) for _ in (0, 1)]
        # a second calc stream (SLF_CALC_STREAMS=1: off).  z / y decompositions sweep their face layers on it: the
        # interior depends on the neighbours only through the face layers of the step before, so its stream never waits
        # for a transfer.  x decompositions alternate their z-chunks between the two streams: a chunk starts while the
        # one before it drains.  Ghost-layer PBC kernels and the macro pass of the non-local models work on whole
        # arrays: one stream there.
        two = os.environ.get('SLF_CALC_STREAMS', '2') != '1' and not self._pbc_axes and not self.has_macro_exchange and \
            bool(self._links) and hasattr(b, 'supports_step_plans') and not self._time_dependent()
        # (time-dependent boundary values are rewritten on the calc stream before every step: every sweep launch on it)
        if self._xface is not None:
            # z-chunks on alternating streams only on request: measured slower than the drain at the chunk boundaries
            # it avoids (profiles/r04/NOTES.md)
            two = two and not self._xface.needs_clear and os.environ.get('SLF_XFACE_STREAMS', '1') == '2'
            n = len(self._xchunks.order)
            self._ev_chunk = [[b.make_event(self._calc_stream) for _ in range(n)] for _ in (0, 1)]
            self._ev_batch = [[b.make_event(self._data_stream) for _ in range(n)] for _ in (0, 1)]
        else:
            two = two and bool(self._regions[0])
        self._bnd_stream = b.make_stream() if two else self._calc_stream

    def _sweep_kernels(self, it, sync_req):
        kernels = self._kernels_full if sync_req else self._kernels_none
        return kernels.primary if (it & 1) == 0 else kernels.secondary

    _step_parity = None       # of the step last enqueued; None: none since the state was written from the host

    def _set_step_state(self, it):
        """What the rest of the runner reads about the step being enqueued (halo_messages, xface_pieces, materialise)."""
        self._step_parity = it & 1

    # in place the even steps pull, every other step pushes; the copy of the arrays the step writes; its z-chunk batches
    _step_pulls = property(lambda self: self._step_parity is not None and
                           xface.step_kinds(self.config.access_pattern == 'AA', self._step_parity)[0] == 'own')
    _step_copy = property(lambda self: 0 if self.config.access_pattern == 'AA' else 1 - self._step_parity)
    _xface_kind = property(lambda self: 'own' if self._step_pulls else 'push')

    def _program(self, q, it, sync_req):
        """One step of a runner that owns its process (reference subdomain_runner.py:960-1058): macro pass of the
        non-local models, sweep, halo -- the exchanges through the connector."""
        self._set_step_state(it)
        self._program_macro(q, it, sync_req=sync_req)
        self._program_front(q, it, sync_req)
        self._program_back(q, it)

    def _neighbour_events(self, group, name, parity):
        """Events `name` of parity `parity` of the runners this one exchanges halos with (same-process groups)."""
        ids = set(self._links) | set(self._macro_links)
        return [group.by_id[nid]._pev[parity][name] for nid in sorted(ids) if nid in group.by_id]

    def _program_macro(self, q, it, group=None, sync_req=False):
        """Macroscopic-field pass of the non-local models (NNSubdomainRunner); nothing here."""

    def _program_macro_back(self, q, it):
        pass

    def _program_front(self, q, it, sync_req, group=None):
        """[face layers -> event] -> interior -> ghost-layer PBC kernels on the calc stream(s); pack on the data stream.
        group: the controller.LocalGroup that steps this runner together with its neighbours in one process -- the group
        moves the packed buffers itself, between the fronts and the backs of its runners; None: the connector does, right
        here (x-face pieces: after every z-chunk)."""
        prof, timed = self._profile, not q.planned
        ev, pev = self._pev[it & 1], self._pev[1 - (it & 1)]
        kernels = self._sweep_kernels(it, sync_req)
        if self._xface is not None:
            return self._program_xface(q, it, kernels, group)
        sk, sb = self._calc_stream, self._bnd_stream
        bnd, bulk = self._regions
        ready = None
        if bnd:
            if self._links:
                q.wait(sb, pev['halo'])
            if sb is not sk:
                q.wait(sb, pev['bulk'])
            if timed:
                prof.record_gpu_start(TimeProfile.BOUNDARY, sb)
            for reg in bnd:
                for k in kernels:
                    q.launch(k, reg, sb)
            if timed:
                prof.record_gpu_end(TimeProfile.BOUNDARY, sb)
            q.record(ev['bnd'], sb)
            if sb is not sk:
                q.wait(sk, pev['bnd'])
            ready = ev['bnd']
        elif self._links:
            q.wait(sk, pev['halo'])
        self._program_sweep_rest(q, it, kernels, bulk, ready, group)
        if bnd and sb is not sk and sync_req:
            # the host is about to look at this step's results (fields to the host, the invalid-value poll, kernels a
            # simulation enqueues from after_step() -- all on the calc stream): they come after the face layers too
            q.wait(sk, ev['bnd'])

    def _program_sweep_rest(self, q, it, kernels, bulk, ready, group):
        prof, timed = self._profile, not q.planned
        ev = self._pev[it & 1]
        sk = self._calc_stream
        if timed:
            prof.record_gpu_start(TimeProfile.BULK, sk)
        for k in kernels:
            q.launch(k, bulk, sk)
        if timed:
            prof.record_gpu_end(TimeProfile.BULK, sk)
        base = 1 - (it & 1)
        for axis in self._pbc_axes:
            for k in self._dist_pbc_kernels()[base][axis]:
                q.launch(k, None, sk)
        q.record(ev['bulk'], sk)
        if ready is None or self._pbc_axes:
            ready = ev['bulk']       # unsplit subdomains: the whole sweep (and the local PBC) must be done first
        self._program_pack(q, it, ready, group)

    def _dist_pbc_kernels(self):
        return self._pbc_kernels

    def _program_pack(self, q, it, ready, group, kind='dist'):
        """Data stream: wait(`ready`) -> pack -> event 'packed'; without a group the exchange follows at once."""
        links = self._links if kind == 'dist' else self._macro_links
        if not links:
            return
        prof, timed, sh = self._profile, not q.planned, self._data_stream
        ev = self._pev[it & 1]
        pre = '' if kind == 'dist' else 'macro_'
        q.wait(sh, ready)
        if group is not None:
            # a send buffer is not written again before the neighbours' copies of the previous step have read it
            for e in self._neighbour_events(group, pre + 'copied', 1 - (it & 1)):
                q.wait(sh, e)
        tp = TimeProfile.COLLECTION if kind == 'dist' else TimeProfile.MACRO_COLLECTION
        if timed:
            prof.record_gpu_start(tp, sh)
        for nid in sorted(links):
            for pack in links[nid].packs[it & 1]:
                q.launch(pack, None, sh)
        if timed:
            prof.record_gpu_end(tp, sh)
        q.record(ev[pre + 'packed'], sh)
        if group is None:
            if timed and kind == 'dist':
                prof.record_cpu_start(TimeProfile.RECV_DISTS)
            self._connector.enqueue_exchange(q, self, kind)
            if timed and kind == 'dist':
                prof.record_cpu_end(TimeProfile.RECV_DISTS)

    def _program_back(self, q, it):
        """Data stream: unpack what the exchange delivered -> event 'halo' (the next step's face layers wait for it)."""
        if not self._links or self._xface is not None:
            return
        prof, timed, sh = self._profile, not q.planned, self._data_stream
        if timed:
            prof.record_gpu_start(TimeProfile.DISTRIB, sh)
        for nid in sorted(self._links):
            for unpack in self._links[nid].unpacks[it & 1]:
                q.launch(unpack, None, sh)
        if timed:
            prof.record_gpu_end(TimeProfile.DISTRIB, sh)
        q.record(self._pev[it & 1]['halo'], sh)

    def _program_xface(self, q, it, kernels, group=None):
        """1-D x decomposition: the sweep in z-chunks; after each chunk the planes of the face buffers that are now
        complete travel on the data stream (own process: through the connector, right here; same-process group: the
        group copies them after the fronts of all its runners).  A chunk waits for the transfers of the previous step
        that carry the planes it reads (xface.ChunkPlan); with SLF_XFACE_STREAMS=2 the chunks alternate between the two
        calc streams and also wait for the chunks of the previous step that touched their planes or their neighbours."""
        prof, timed = self._profile, not q.planned
        x, plan = self._xface, self._xchunks
        par = it & 1
        kind, prev_kind = xface.step_kinds(self.config.access_pattern == 'AA', it)
        ny = list(reversed(self._lat_size))[1] - 2
        streams = [self._calc_stream, self._bnd_stream]
        snd, rcv = x.send[par], x.recv[1 - par]
        # every sweep of the group on one stream (controller.LocalGroup._serialise_sweeps): its order is all the order
        # the shared face buffers need -- no events
        serial = group is not None and getattr(group, 'single_calc_stream', False) and x.shared
        if group is not None and not serial:
            # the send set of this parity was last read by the neighbours' copies of step it - 2
            for e in self._neighbour_events(group, 'copied', par):
                q.wait(streams[0], e)
        q.xface(self.module, snd[xface.LOW], snd[xface.HIGH], rcv[xface.LOW], rcv[xface.HIGH])
        if x.needs_clear:
            for a in snd:
                if a:
                    q.memset(a, 0xFF, x.nbytes, streams[0])
        if timed:
            prof.record_gpu_start(TimeProfile.BULK, streams[0])
        if serial:
            for pos, c in enumerate(plan.order):
                for k in kernels:
                    q.launch(k, plan.region(c, ny), streams[pos & 1])
        else:
            events = (self._ev_chunk[par], self._ev_batch[par], self._ev_chunk[1 - par], self._ev_batch[1 - par])
            # face buffers that are not copied (the neighbour's receive planes ARE my send planes: peer transport, subdomains
            # of one process): a chunk also waits until the planes it writes have been read (xface.ChunkPlan.peer_need)
            need = plan.peer_need(kind, prev_kind) if x.shared else plan.need[prev_kind]
            every = x.shared and group is None      # a signal after every chunk: the neighbours' chunks count on it

            def exchange(pos):
                self._connector.enqueue_pieces(q, self, self.xface_pieces(pos))
            # (a group copies the planes itself, after the fronts of all its runners)
            xface.program_chunks(q, plan, ny, kernels, streams, self._data_stream, events, need, every,
                                 exchange if group is None else None)
        if timed:
            if streams[1] is not streams[0]:
                streams[0].wait_for_event(self._ev_chunk[par][len(plan.order) - 1])
            prof.record_gpu_end(TimeProfile.BULK, streams[0])

    # ------------------------------------------------------------------ force objects (lb_base.ForceObject)
    _fo_tables = None

    def _init_force_objects(self):
        """Link tables of the simulation's force objects on the device (reference subdomain_runner.py:1459-1509): per link
        the two words of the distribution array of lattice 0 that hold the populations crossing it after propagation, and its
        direction.  Links in the reference's order -- objects, ascending direction, np.where order of the solid node --
        whatever the access pattern and the addressing mode; all objects of the subdomain share one set of tables, object k
        owning the links seg[k] .. seg[k + 1] - 1.

        Word indices.  Link "solid node s, direction i, fluid node f = s + e_i": the reference reads dist[opp(i)][s] +
        dist[i][f] of the copy the last step wrote.  In the in-place pattern the array is in that natural order after an
        even number of steps; after an odd number the post-propagation value of direction k at node x sits in slot opp(k)
        at x - e_k, which puts the first term at (i, f) and the second at (opp(i), s): the same two words.  One table
        serves both patterns and both parities."""
        sim, sub = self._sim, self._subdomain
        if not sim.force_objects:
            return
        cfg = self.config
        if int(self._desc.lattice) in (hipabi.SLF_D3Q15, hipabi.SLF_D3Q27):
            raise NotImplementedError('%s: force objects are not implemented on this lattice' % sim.grid.__name__)
        if len(sim.grids) != 1 or int(self._desc.simtype) != hipabi.SLF_SIM_LBM:
            raise NotImplementedError('force objects: single-fluid simulations only (the momentum exchange is read off one '
                                      'lattice; Shan-Chen and binary models are not covered)')
        if getattr(cfg, 'minimize_roundoff', False):
            raise NotImplementedError('force objects with --minimize_roundoff: the arrays hold f - w, not the populations')
        if not hasattr(self.backend, 'force_objects'):
            raise NotImplementedError('force objects: backend %s has no force_objects()' % getattr(self.backend, 'name', '?'))
        cfg.logger.info('Processing force objects.')
        grid, es = sim.grid, self._spec.envelope_size
        stride, phys = self._dist_stride, self._physical_size
        addr = self._host_indirect_address.reshape(-1) if self.indirect else None
        idx, idx2, dirs, seg, live = [], [], [], [0], []
        for fo in sim.force_objects:
            dists = sub.get_fo_distributions(fo)
            leaving = sub.fo_links_leaving(fo)
            for dist_num, locs in sorted(dists.items()):
                if leaving is not None:
                    break
                vec = grid.basis[dist_num]
                for axis in range(self.dim):
                    p = locs[self.dim - 1 - axis] + int(vec[axis])
                    out = (p < es) | (p >= es + self._spec.size[axis])
                    if out.any():
                        k = int(np.nonzero(out)[0][0])
                        where = tuple(int(locs[self.dim - 1 - a][k]) - es + self._spec.location[a] for a in range(self.dim))
                        leaving = (dist_num, sub.FACE_NAMES[2 * axis + int(p[k] >= es)], where)
                        break
            if leaving is not None:
                raise NotImplementedError(
                    '%s (box %s .. %s): the link from the solid node %s along direction %d leaves subdomain %d through its '
                    'face %s.  Momentum links across subdomain seams, periodic faces or the ghost layer are not supported: '
                    'keep the object inside one subdomain and away from periodic faces.'
                    % (fo, tuple(fo.start), tuple(fo.end), leaving[2], leaving[0], self._spec.id, leaving[1]))
            if not dists:
                cfg.logger.warning('No momentum-transferring distributions found for %s' % fo)
                continue
            for dist_num, locs in sorted(dists.items()):
                vec = grid.basis[dist_num]
                solid = np.ravel_multi_index(locs, phys).astype(np.int64)
                fluid = np.ravel_multi_index(tuple(l + int(c) for l, c in zip(locs, reversed(vec))), phys).astype(np.int64)
                if addr is not None:
                    solid, fluid = addr[solid].astype(np.int64), addr[fluid].astype(np.int64)
                    if (solid == hipabi.SLF_INVALID_NODE).any() or (fluid == hipabi.SLF_INVALID_NODE).any():
                        raise ValueError('%s: a momentum link ends at a node that owns no slot in the distribution arrays '
                                         '(the active-node map leaves out a solid node next to a fluid node)' % fo)
                idx.append(grid.idx_opposite[dist_num] * stride + solid)       # momentum transferred to the solid node
                idx2.append(dist_num * stride + fluid)                         # ... and from it
                dirs.append(np.full(solid.size, dist_num, dtype=np.uint8))
            seg.append(seg[-1] + sum(l[0].size for l in dists.values()))
            fo.num_links = seg[-1] - seg[-2]
            cfg.logger.debug('%s: total momentum links: %d' % (fo, fo.num_links))
            live.append(fo)
        if not live:
            return
        idx, idx2, dirs = np.concatenate(idx), np.concatenate(idx2), np.concatenate(dirs)
        words = grid.Q * stride
        assert idx.min() >= 0 and idx2.min() >= 0 and idx.max() < words and idx2.max() < words < 2 ** 32
        b = self.backend
        t = self._fo_tables = {'n': len(live), 'max_links': int(np.diff(seg).max()), 'objects': live,
                               'host': (idx.astype(np.uint32), idx2.astype(np.uint32), dirs, np.array(seg, dtype=np.uint32)),
                               'out_host': np.zeros(3 * len(live), dtype=np.float64)}
        t['idx'], t['idx2'], t['dirs'], t['seg'] = [b.alloc_buf(like=a) for a in t['host']]
        t['out'] = b.alloc_buf(like=t['out_host'])
        t['workspace'] = b.force_workspace(self.module, t['n'], t['max_links'])
        for k, fo in enumerate(live):
            # the object's dim doubles inside the result array: from_buf(fo.gpu_force_buf) fills fo.force_buf
            fo.force_buf = np.zeros(self.dim, dtype=np.float64)
            fo.gpu_force_buf = t['out'] + 24 * k
            b.buffers[fo.gpu_force_buf] = fo.force_buf

    def update_force_objects(self):
        """Enqueues, on the calc stream and without a host wait, the sums of all initialised force objects of this
        subdomain from the populations as they are after the last completed step (they are read AFTER propagation,
        reference subdomain_runner.py:1512-1526).  Read a result with backend.from_buf(fo.gpu_force_buf)."""
        t = self._fo_tables
        if t is None:
            return
        calc = self._calc_stream
        for s in self._all_streams():
            if s is not calc:         # whatever part of the step ran on another stream comes first
                calc.wait_for_event(self.backend.make_event(s))
        self.backend.force_objects(self.module, self.gpu_dist(0, self._sim.iteration & 1), t['idx'], t['idx2'], t['dirs'],
                                   t['seg'], t['n'], t['max_links'], t['workspace'], t['out'], calc)
        pending = getattr(self.backend, 'buffer_streams', None)
        if pending is not None:       # from_buf() of a result waits for the stream that produces it, and for nothing else
            for fo in t['objects']:
                pending[fo.gpu_force_buf] = calc

    # ------------------------------------------------------------------ data movement
    def _fields_to_host(self, sync=True):
        bs = getattr(self, '_bnd_stream', None)
        if bs is not None and bs is not self._calc_stream:
            bs.synchronize()            # the face layers / every other z-chunk stored their fields on the second stream
        for field in self._scalar_fields:
            self.backend.from_buf_async(self.gpu_field(field), self._calc_stream)
        for vec in self._vector_fields:
            for comp in vec:
                self.backend.from_buf_async(self.gpu_field(comp), self._calc_stream)
        if sync:
            self.backend.sync_stream(self._calc_stream)

    def _fields_to_gpu(self):
        for field in self._scalar_fields:
            self.backend.to_buf(self.gpu_field(field))
        for vec in self._vector_fields:
            for comp in vec:
                self.backend.to_buf(self.gpu_field(comp))

    def _debug_get_dist(self, output=True, grid_num=0, copy=None):
        """Distributions as [Q, (nz,) ny, arr_nx] (reference subdomain_runner.py:1363-1381); with indirect
        addressing the slots are scattered back to their nodes (inactive nodes: 0)."""
        self.backend.sync_stream(*self._all_streams())
        self._halo.materialise()
        if copy is None:
            copy = 0 if not self._gpu_grids_secondary else (self._sim.iteration & 1)
        raw = np.zeros((self._sim.grid.Q, self._dist_stride), dtype=self.float)
        self.backend.from_buf(self.gpu_dist(grid_num, copy), raw)
        if self.indirect:
            addr = self._host_indirect_address.reshape(-1)
            act = addr != hipabi.SLF_INVALID_NODE
            dense = np.zeros((self._sim.grid.Q, self._get_nodes()), dtype=self.float)
            dense[:, act] = raw[:, addr[act]]
            return dense.reshape([self._sim.grid.Q] + self._physical_size)
        return np.ascontiguousarray(raw[:, :self._get_nodes()]).reshape([self._sim.grid.Q] + self._physical_size)

    def _debug_set_dist(self, dbuf, output=True, grid_num=0, copy=None):
        if copy is None:
            copy = 0 if not self._gpu_grids_secondary else (self._sim.iteration & 1)
        raw = np.zeros((self._sim.grid.Q, self._dist_stride), dtype=self.float)
        dense = np.asarray(dbuf, dtype=self.float).reshape(self._sim.grid.Q, -1)
        if self.indirect:
            addr = self._host_indirect_address.reshape(-1)
            act = addr != hipabi.SLF_INVALID_NODE
            raw[:, addr[act]] = dense[:, act]
            raw[:, self._subdomain.active_nodes:] = np.nan       # the spare slot: never written (_alloc_distributions)
        else:
            raw[:, :self._get_nodes()] = dense
        self.backend.to_buf(self.gpu_dist(grid_num, copy), raw)
        if isinstance(getattr(self, '_resident', None), dict):
            self._resident['equalised'] = False      # the scratch copies of the resident launches no longer agree with the arrays
        self._halo.reset()

    def _debug_global_idx_to_tuple(self, gi):
        dist_num = gi // self._get_nodes()
        dist_idx = gi % self._get_nodes()
        return (dist_num,) + tuple(np.unravel_index(dist_idx, self._physical_size))

    def save_checkpoint(self):
        """<base>.<iter>.<subdomain>.cpoint.npz with the simulation state and dist<N>a[/dist<N>b] of every
        lattice N (reference :1414-1431; --single_checkpoint keeps one file that is overwritten)."""
        if getattr(self.config, 'single_checkpoint', False):
            fname = io.checkpoint_filename(self.config.checkpoint_file, 1, self._spec.id, 0)
        else:
            fname = io.checkpoint_filename(self.config.checkpoint_file, io.filename_iter_digits(self.config.max_iters),
                                           self._spec.id, self._sim.iteration)
        data = {'state': np.frombuffer(pickle.dumps(self._sim.get_state()), dtype=np.uint8)}
        cur = (self._sim.iteration & 1) if self._gpu_grids_secondary else 0
        for n in range(len(self._gpu_grids_primary)):
            # dist<N>a = gpu_dist(N, iteration & 1): the current state; dist<N>b the other copy (reference :1420-1427)
            data['dist%da' % n] = self._debug_get_dist(grid_num=n, copy=cur)
            if self._gpu_grids_secondary:
                data['dist%db' % n] = self._debug_get_dist(grid_num=n, copy=1 - cur)
        # fields that are STATE, not output derived from the populations (LBSim.checkpoint_fields: the alpha field of
        # the entropic collision, whose entries are the Newton start values of the next step)
        for name in getattr(self._sim, 'checkpoint_fields', ()):
            host = getattr(self._sim, name)
            self.backend.from_buf(self.gpu_field(host))
            data['field_' + name] = np.array(host)
        np.savez(fname, **data)

    def restore_checkpoint(self, fname):
        self.config.logger.info('Restoring checkpoint from {0}'.format(fname))
        cpoint = np.load(fname, allow_pickle=False)
        state = pickle.loads(cpoint['state'].tobytes())
        saved_it = int(state.get('iteration', 0)) if isinstance(state, dict) else 0
        # the simulation state is always restored (subclass state lives there); without --restore_time only the
        # clock is reset afterwards (reference :1436-1449)
        self._sim.set_state(state)
        if not getattr(self.config, 'restore_time', True):
            self._sim.iteration = 0
        it = self._sim.iteration
        if not self._gpu_grids_secondary and (saved_it & 1) != (it & 1):
            raise ValueError('AA checkpoint written at iteration %d cannot be continued from iteration %d: the in-place '
                             'pattern stores the populations in a layout that depends on the parity of the step'
                             % (saved_it, it))
        cur = (it & 1) if self._gpu_grids_secondary else 0
        for key in cpoint.files:
            if not key.startswith('dist'):
                continue
            n, is_a = int(key[4:-1]), key.endswith('a')
            if n >= len(self._gpu_grids_primary) or (not is_a and not self._gpu_grids_secondary):
                continue
            self._debug_set_dist(cpoint[key], grid_num=n, copy=cur if is_a else 1 - cur)
        for name in getattr(self._sim, 'checkpoint_fields', ()):
            if 'field_' + name in cpoint.files:
                host = getattr(self._sim, name)
                host[...] = cpoint['field_' + name]
                self.backend.to_buf(self.gpu_field(host))
        self.backend.set_iteration(self._sim.iteration)

    # ------------------------------------------------------------------ life cycle
    def sighup_handler(self, signum, frame):
        self.config.logger.info('Received HUP signal, will save checkpoint (it=%d).' % self._sim.iteration)
        self._checkpoint_req = True

    def _install_signal_handlers(self):
        import signal
        import threading
        if hasattr(signal, 'SIGHUP') and threading.current_thread() is threading.main_thread():
            # several runners in one process: every one gets the request.  One handler for the process and a weak set of
            # runners -- a handler per runner that calls the one before it grows by a frame with every simulation the
            # process has run (and keeps their runners alive): after a thousand of them SIGHUP ended in a RecursionError.
            _hup_runners.add(self)
            current = signal.getsignal(signal.SIGHUP)
            if current is not _hup_dispatch:
                _hup_state['previous'] = current
                signal.signal(signal.SIGHUP, _hup_dispatch)

    def prepare(self):
        """Everything up to (not including) the main loop (reference run(), :1537-1602)."""
        cfg = self.config
        self._install_signal_handlers()
        self._init_geometry()
        self._sim.init_fields(self)
        self._init_compute()
        self._subdomain.init_fields(self._sim)
        self._sim.verify_fields()
        self._init_gpu_data()
        self._init_force_objects()
        self._init_halo()
        self._prepare_compute_kernels()
        self._init_step_program()
        self._gpu_initial_conditions()
        self.backend.set_iteration(0)
        if self._output is not None:
            self._output.set_fluid_map(self._subdomain.fluid_map())
        if getattr(cfg, 'restore_from', ''):
            fname = io.subdomain_checkpoint(cfg.restore_from, self._spec.id)
            self.restore_checkpoint(fname)
        if getattr(cfg, 'debug_dump_node_type_map', False) and self._output is not None:
            self._output.dump_node_type(self._subdomain._type_vis_map)
        self._halo.reset()
        self._sim.before_main_loop(self)
        # mix-ins have before_main_loop routines of their own (reference subdomain_runner.py:1590-1594): a simulation
        # that overrides the hook, as the reference's kida_vortex.py does, need not call them
        for c in type(self._sim).mro()[1:]:
            if issubclass(c, LBMixIn) and not issubclass(c, LBSim) and 'before_main_loop' in vars(c):
                c.before_main_loop(self._sim, self)
        self.backend.sync_stream(self._calc_stream)
        self.num_fluid_nodes = self._subdomain.num_fluid_nodes

    def _gpu_initial_conditions(self):
        """The distributions from the macroscopic fields the subdomain's initial_conditions() wrote."""
        self._sim.initial_conditions(self)

    def need_quit(self):
        cfg = self.config
        if cfg.max_iters > 0 and self._sim.iteration >= cfg.max_iters:
            return True
        return self._quit_event is not None and self._quit_event.is_set()

    def pre_step(self):
        """Returns (sync_req, output_req) for the coming step (reference main(), :1668-1712)."""
        output_req = self._sim.need_output()
        last = self.config.max_iters > 0 and self._sim.iteration + 1 >= self.config.max_iters
        sync_req, fields_req = self._sim.need_sync_fields()
        if last:
            sync_req = fields_req = True
        return sync_req, fields_req, output_req

    def check_gpu_invalid(self):
        """On-GPU invalid value check (reference --check_invalid_results_gpu): the sweeps flag wet nodes with
        a non-finite density; polled whenever the host synchronises with the device anyway."""
        # (the entropic collision raises the same word where its Newton iteration gives up, whatever the option says)
        if not getattr(self.config, 'check_invalid_results_gpu', False) and getattr(self.config, 'model', '') != 'elbm':
            return
        pos = self.backend.poll_invalid(self.module, self._calc_stream)
        if pos is not None:
            gpos = [int(p) - 1 + o for p, o in zip(pos, self._spec.location)]
            raise self.backend.FatalError(
                'Invalid value (inf / nan%s) detected on the GPU: subdomain %d, node %s (global position %s), '
                'before iteration %d' % (', or an entropic collision whose alpha iteration did not converge'
                                         if getattr(self.config, 'model', '') == 'elbm' else '',
                                         self._spec.id, tuple(pos[:self.dim]), tuple(gpos), self._sim.iteration))

    def post_step(self, sync_req, output_req):
        cfg = self.config
        if sync_req:
            self.check_gpu_invalid()
            self._fields_to_host(True)
            if getattr(cfg, 'check_invalid_results_host', True) and self._output is not None and \
                    self._output._fluid_map is not None and not self._output.verify():
                raise RuntimeError('Invalid value detected in output for iteration %d' % self._sim.iteration)
        if output_req and cfg.output_required and self._output is not None:
            if cfg.output:
                self._output.save(self._sim.iteration)
            if getattr(cfg, 'debug_dump_dists', False):
                self._output.dump_dists([self._debug_get_dist()], self._sim.iteration)
        if (self._sim.need_checkpoint() or self._checkpoint_req) and cfg.checkpoint_file:
            self._checkpoint_req = False
            self.save_checkpoint()
        self._sim.after_step(self)

    # ------------------------------------------------------------------ launch graphs
    GRAPH_STEPS = (16, 2)      # graph sizes (steps per replay), largest first; even -> the AA parity repeats

    def _enqueue_plain_step(self, it):
        """The kernels of one step without output, halo or profiling (what a graph records)."""
        b = self.backend
        kernels = self._kernels_none.primary if (it & 1) == 0 else self._kernels_none.secondary
        for k in kernels:
            b.run_kernel(k, self._regions[1], self._calc_stream)
        base = 1 - (it & 1)
        for axis in self._pbc_axes:
            for k in self._pbc_kernels[base][axis]:
                b.run_kernel(k, None, self._calc_stream)

    def _steps_without_host(self):
        """Number of coming steps that need no host involvement at all: no output, field transfer,
        checkpoint, statistics line, user hook or end-of-run handling."""
        cfg, sim = self.config, self._sim
        it = sim.iteration
        if type(sim).after_step is not LBSim.after_step or sim.need_sync_flag or sim.need_fields_flag or \
                self._checkpoint_req:
            return 0
        lim = [1 << 30]
        if cfg.max_iters > 0:
            lim.append(cfg.max_iters - 1 - it)          # the final step transfers the fields
        if cfg.output_required:
            every = max(1, int(cfg.every))
            first = max(it, int(getattr(cfg, 'from_', 0)))
            nxt = first + ((every - 1 - first) % every)    # first s >= first with (s + 1) % every == 0
            lim.append(nxt - it)
        if getattr(cfg, 'checkpoint_every', 0) > 0 and cfg.checkpoint_file:
            lim.append(cfg.checkpoint_every - 1 - (it % cfg.checkpoint_every))
        if cfg.perf_stats_every > 0:
            lim.append(cfg.perf_stats_every - 1 - (it % cfg.perf_stats_every))
        prof = self._profile
        if prof._is_benchmark and it < prof._sample_from:
            lim.append(prof._sample_from - it)             # sampling starts exactly there
        return max(0, min(lim))

    # ------------------------------------------------------------------ several steps per launch (small 2-D subdomains)
    RESIDENT_STEPS = {'AA': 8, 'AB': 7}       # steps per launch: a halo of 8 nodes either way (csrc/slf_resident.hip)
    RESIDENT_LAUNCHES = (16, 2)               # launches per graph replay, largest first; even: the result is back in the arrays
    RESIDENT_MAX_NODES = 90000                # beyond this a launch per step is faster (measured, see _resident_setup)
    _resident = None

    @staticmethod
    def resident_halo(aa, steps):
        """Halo the tiles of a launch of `steps` steps need, whatever the parity of its first step (the library checks)."""
        return 2 * ((steps + 1) // 2) if aa else steps + 1

    def _resident_setup(self):
        """Kernels, scratch copies and tile shape of the several-steps-per-launch path, or None where it does not apply:
        2-D single-fluid subdomains without neighbours, small enough to be launch-bound, periodic axes wrapped in-sweep,
        node kinds the library's resident kernel serves (it refuses the others)."""
        if self._resident is not None:
            return self._resident or None
        self._resident = False
        cfg, sim, b = self.config, self._sim, self.backend
        if self.dim != 2 or not getattr(cfg, 'hip_resident', True) or os.environ.get('SLF_RESIDENT', '1') == '0' or \
                not hasattr(sim, 'get_resident_kernels') or self._pbc_axes or self.indirect or len(sim.grids) != 1 or \
                self._links or self.has_macro_exchange or getattr(sim, 'has_accel_field', False):
            return None                 # (an acceleration field is read by the per-node sweep only)
        d = self._desc
        ext = [(d.lat_nx - 2) if d.periodic_fused[0] else d.lat_nx, (d.lat_ny - 2) if d.periodic_fused[1] else d.lat_ny]
        # Where it pays (256^2 cavity on MI355X, GMLUPS with / without, profiles/r05/ldc2d_resident_variants.txt): in place
        # 17.5 / 13.7, two-copy 16.9 / 12.6, MRT 15.8 / 13.2, 128^2 5.2 / 3.6 -- and where it does not: 512^2 23.8 / 33.6 (the
        # windows hold 4 x the nodes and the launch is bound by instruction issue, so its time grows with the subdomain while
        # a plain sweep of that size is still near its launch-bound plateau), double precision 7.2 / 11.0 (twice the LDS
        # traffic, half the vector rate).  SLF_RESIDENT_FORCE=1 takes the path wherever the kernel applies (the tests).
        if os.environ.get('SLF_RESIDENT_FORCE', '0') != '1':
            if ext[0] * ext[1] > int(os.environ.get('SLF_RESIDENT_MAX_NODES', self.RESIDENT_MAX_NODES)) or \
                    self.float().itemsize != 4:
                return None
        aa = cfg.access_pattern == 'AA'
        steps = int(os.environ.get('SLF_RESIDENT_STEPS', self.RESIDENT_STEPS[cfg.access_pattern]))
        halo = self.resident_halo(aa, steps)
        isz = self.float().itemsize
        # tiles: at most 16 x 16 of them (one workgroup per CU on 256 CUs), windows of at most 2048 nodes in 160 KiB of LDS
        tile = [max(1, -(-e // 16)) for e in ext]
        while (tile[0] + 2 * halo) * (tile[1] + 2 * halo) > 2048 or \
                (tile[0] + 2 * halo) * (tile[1] + 2 * halo) * (9 * isz * 2 + 8) + 4352 > 160 * 1024:   # + the kernel's static tables
            a = 0 if tile[0] >= tile[1] else 1
            if tile[a] == 1:
                return None
            tile[a] -= 1
        nbytes = sim.grid.Q * self._dist_stride * isz
        off = b.dist_align_offset(isz)
        scratch = [b.alloc_buf(size=nbytes, align_offset=off), 0 if aa else b.alloc_buf(size=nbytes, align_offset=off)]
        try:
            fwd, bwd = sim.get_resident_kernels(self, scratch, steps, tile, halo)
        except b.FatalError as e:       # node kinds / formulations the resident kernel does not serve
            cfg.logger.debug('several steps per launch not available: %s' % e)
            for addr in scratch:
                if addr:
                    b.free_buf(addr)
            return None
        pairs = [(self.gpu_dist(0, 0), scratch[0])] + ([] if aa else [(self.gpu_dist(0, 1), scratch[1])])
        self._resident = dict(steps=steps, halo=halo, tile=tile, fwd=fwd, bwd=bwd, pairs=pairs, nbytes=nbytes, graphs={})
        cfg.logger.debug('several steps per launch: %d steps, tiles %s, halo %d' % (steps, tile, halo))
        return self._resident

    def _fast_forward_resident(self, n):
        """As many of the coming n host-free steps as whole graphs of resident launches cover.  Returns the steps done."""
        r = self._resident_setup()
        if r is None or n < 2 * r['steps']:
            return 0
        b, stream = self.backend, self._calc_stream

        def enqueue(start, count):
            def launches():
                for j in range(count):
                    b.set_iteration(start + j * r['steps'])
                    b.run_kernel(r['fwd'] if (j & 1) == 0 else r['bwd'], None, stream)
            return launches

        def give_up(e):
            self.config.logger.warning('HIP graph capture of the resident launches failed (%s)' % e)
            # the path is given up for good: its scratch copies of the arrays and the graphs go with it
            b.sync_stream(stream)
            r['graphs'].clear()
            for _, scratch in r['pairs']:
                b.free_buf(scratch)
            self._resident = False

        def equalise():
            # what no tile covers (padding, the ghost columns of an axis wrapped in-sweep) is the same in both buffers: no
            # kernel ever writes there, so once is enough -- until the host rewrites the arrays (_debug_set_dist clears
            # the flag)
            if not r.get('equalised'):
                for dist, scratch in r['pairs']:
                    b.copy_buf_async(scratch, dist, r['nbytes'], stream)
                r['equalised'] = True
        return self._replay_graphs(n, 0, self.RESIDENT_LAUNCHES, r['steps'], r['graphs'], stream, enqueue, give_up, equalise)

    def _replay_graphs(self, n, done, sizes, steps, graphs, stream, enqueue, capture_failed, before_first=None):
        """Of the coming n host-free steps, `done` of which are behind us already: as many as whole graphs cover.  sizes:
        launches per graph, largest first, `steps` steps each; graphs: {(launches, parity of the first step): graph},
        captured on first use from enqueue(first step, launches) on `stream`.  A capture that fails ends the loop after
        capture_failed(error).  before_first(): once, in front of the first launch.  Returns the steps done in all."""
        b, prof = self.backend, self._profile
        it = self._sim.iteration - done
        for count in sizes:
            size = count * steps
            while n - done >= size:
                key = (count, (it + done) & 1)
                if key not in graphs:
                    try:
                        graphs[key] = b.capture_graph(stream, enqueue(it + done, count))
                    except b.FatalError as e:
                        capture_failed(e)
                        b.set_iteration(self._sim.iteration)
                        return done
                if before_first is not None:
                    before_first()
                    before_first = None
                prof.start_step()
                prof.record_gpu_start(TimeProfile.BULK, stream)
                graphs[key].launch(stream)
                prof.record_gpu_end(TimeProfile.BULK, stream, steps=size)
                done += size
                self._sim.iteration = it + done
                prof.end_step(size)
        b.set_iteration(self._sim.iteration)
        return done

    def fast_forward(self):
        """Replays as many of the coming steps as possible as HIP graphs (launch-bound small
        subdomains: one runtime call per 2 / 16 steps instead of a Python-level launch per kernel); small 2-D subdomains
        go through launches that perform several steps each (_fast_forward_resident) first.
        Returns the number of steps done (0: take a normal step)."""
        if not getattr(self.config, 'hip_graphs', True) or self._links or self._quit_requested() or self._time_dependent():
            return 0         # (time-dependent boundary values: the host writes them before every step)
        n = self._steps_without_host()
        if n < 2:
            return 0
        b = self.backend
        done = self._fast_forward_resident(n)

        def enqueue(start, count):
            def steps():
                for s_ in range(start, start + count):
                    b.set_iteration(s_)
                    self._enqueue_plain_step(s_)
            return steps

        def carry_on(e):
            # nothing was executed; carry on with plain launches
            self.config.logger.warning('HIP graph capture failed (%s); continuing without graphs' % e)
            self.config.hip_graphs = False
        return self._replay_graphs(n, done, self.GRAPH_STEPS, 1, self.__dict__.setdefault('_graphs', {}), self._calc_stream,
                                   enqueue, carry_on)

    def _quit_requested(self):
        return self._quit_event is not None and self._quit_event.is_set()

    def _all_streams(self):
        out = [self._calc_stream, self._data_stream]
        bs = getattr(self, '_bnd_stream', None)
        if bs is not None and bs is not self._calc_stream:
            out.append(bs)
        return out

    def finish(self):
        self.backend.sync_stream(*self._all_streams())
        peer = getattr(self._connector, 'peer', None)
        if peer is not None:
            peer.check()        # a wait that gave up (a neighbour that is gone): an error, not wrong numbers
        self.check_gpu_invalid()
        if getattr(self.config, 'final_checkpoint', False) and self.config.checkpoint_file:
            self.save_checkpoint()
        self._sim.after_main_loop(self)
        if self._output is not None:
            self._output.wait()

    def release(self):
        """Gives the device memory of this subdomain back (fields, populations, node map, halo buffers).  The
        runner must not be stepped or queried for device data afterwards; the host copies of the output fields
        (sim.rho, sim.v) stay valid."""
        self.backend.sync_stream(*self._all_streams())
        self._kernels_full = self._kernels_none = self._pbc_kernels = None
        self._halo = halo.Halo()
        if self._connector is not None:
            self._connector.release(self)
        self.backend.close()

    def main(self):
        """Main loop of a runner that owns its process (one subdomain per GPU process)."""
        cfg = self.config
        t_prev = time.time()
        it_prev = self._sim.iteration
        self._profile.record_start()
        while not self.need_quit():
            if self.fast_forward():
                continue
            sync_req, fields_req, output_req = self.pre_step()
            self._profile.start_step()
            self.step(fields_req)
            self.post_step(sync_req, output_req)
            self._profile.end_step()
            if cfg.perf_stats_every > 0 and self._sim.iteration % cfg.perf_stats_every == 0:
                self.backend.sync_stream(*self._all_streams())
                now = time.time()
                mlups = self.num_fluid_nodes * (self._sim.iteration - it_prev) / (now - t_prev) * 1e-6
                cfg.logger.info('iteration:{0}  speed:{1:.2f} MLUPS'.format(self._sim.iteration, mlups))
                t_prev, it_prev = now, self._sim.iteration
        self.summary = self._profile.record_end()
        self.finish()

    def run(self):
        self.prepare()
        t0 = time.time()
        it0 = self._sim.iteration
        self.main()
        self.timing = {'steps': self._sim.iteration - it0, 'wall': time.time() - t0}


class NNSubdomainRunner(SubdomainRunner):
    """Runner for models with non-local interactions (reference subdomain_runner.py:1840-2197): every
    step first computes the macroscopic fields of all nodes, makes them available on the ghost layer
    (periodic boundaries), and only then collides and streams:

        ShanChenPrepareMacroFields -> ApplyMacroPeriodicBoundaryConditions (rho, phi)
        -> ShanChenCollideAndPropagate0, 1 -> ApplyPeriodicBoundaryConditions (both lattices)

    Axes wrapped inside the kernels need no ghost fill.  Between subdomains the fields travel like the populations,
    in an exchange of their own in front of the sweep (reference _send_macro/_recv_macro; sailfish_amd/halo.py)."""

    has_macro_exchange = True

    def _nnx_serial(self, group):
        """Stepped by a group that runs every sweep of its subdomains on ONE stream, planes shared with the neighbours: the
        order of that stream is all the order the planes need (controller.LocalGroup._serialise_sweeps)."""
        return self._nnx is not None and group is not None and getattr(group, 'single_calc_stream', False) and self._nnx.shared

    # ---- start-up of models whose initial conditions read a field at neighbouring nodes (free energy: the Laplacian and
    # the gradient of the host's phi) -- reference NNSubdomainRunner._gpu_initial_conditions, subdomain_runner.py:2079-2100
    _startup_pending = False

    def _startup_needs_fields(self):
        return bool(getattr(self._sim, 'initial_conditions_need_nn', False))

    def _gpu_initial_conditions(self):
        """Fills the ghost layer of the fields the initial conditions read -- local periodic images, then one exchange of
        the fields with the neighbours -- in front of SetInitialConditions.  Shan-Chen models start from every node's own
        values: nothing is exchanged for them.  Subdomains stepped by a same-process group can only exchange once every one
        of them has its fields on the device: the group finishes the start-up after the last prepare()
        (controller.LocalGroup._startup_fields; before_main_loop() hooks of such runners see the arrays before that)."""
        if not self._startup_needs_fields():
            return SubdomainRunner._gpu_initial_conditions(self)
        from sailfish_amd.connector import LocalConnector
        if self._macro_links and isinstance(self._connector, LocalConnector):
            self._startup_pending = True
            return
        q = DirectQueue(self.backend)
        self._set_step_state(0)
        self._program_startup_fields(q)
        self._program_macro_back(q, 0)
        self._finish_startup()

    def _program_startup_fields(self, q, group=None):
        """What _program_macro() does behind the macro pass, for the fields as the host wrote them (parity 0)."""
        sk, ev = self._calc_stream, self._pev[0]
        for axis in self._pbc_axes:
            for k in self._pbc_kernels.macro[1][axis]:
                q.launch(k, None, sk)
        if self._macro_links:
            q.record(ev['macro'], sk)
            self._program_pack(q, 0, ev['macro'], group, kind='macro')

    def _finish_startup(self):
        if not getattr(self.config, 'restore_from', '') or not self._startup_pending:
            SubdomainRunner._gpu_initial_conditions(self)       # (a pending start-up comes after the checkpoint was read)
        self._startup_pending = False
        self._step_parity = None
        self.backend.sync_stream(*self._all_streams())

    def _enqueue_plain_step(self, it):
        b = self.backend
        macro_kernel, sim_kernels = self._kernels_none[it & 1]
        base = 1 - (it & 1)
        b.run_kernel(macro_kernel, None, self._calc_stream)
        for axis in self._pbc_axes:
            for k in self._pbc_kernels.macro[base][axis]:
                b.run_kernel(k, None, self._calc_stream)
        for k in sim_kernels:
            b.run_kernel(k, None, self._calc_stream)
        for axis in self._pbc_axes:
            for k in self._pbc_kernels.distributions[base][axis]:
                b.run_kernel(k, None, self._calc_stream)

    def _dist_pbc_kernels(self):
        return self._pbc_kernels.distributions

    def _sweep_kernels(self, it, sync_req):
        return (self._kernels_full if sync_req else self._kernels_none)[it & 1][1]

    def _program_macro(self, q, it, group=None, sync_req=False):
        """Macroscopic fields of every real node, their local periodic images, and the exchange of the values the
        non-local force reads in the neighbours' territory (reference NNSubdomainRunner.step, subdomain_runner.py:
        2102-2197): calc stream -> event -> data stream: pack -> [exchange] -> unpack -> event -> calc stream."""
        prof, timed = self._profile, not q.planned
        ev, pev = self._pev[it & 1], self._pev[1 - (it & 1)]
        sk = self._calc_stream
        # the kernels of an output step store every field the host reads afterwards (binary Shan-Chen: the velocity,
        # which the other steps' pass leaves to the sweep -- lb_binary.get_compute_kernels)
        macro_kernel = (self._kernels_full if sync_req else self._kernels_none)[it & 1][0]
        base = 1 - (it & 1)
        if self._nnx is not None:
            self._nnx.program_bind(q, it)
            if self._nnx_serial(group):
                q.launch(macro_kernel, None, sk)
                return
        if self._links:
            q.wait(sk, pev['halo'])                          # populations received after the last step
        if timed:
            prof.record_gpu_start(TimeProfile.MACRO_BULK, sk)
        q.launch(macro_kernel, None, sk)
        if timed:
            prof.record_gpu_end(TimeProfile.MACRO_BULK, sk)
        for axis in self._pbc_axes:
            for k in self._pbc_kernels.macro[base][axis]:
                q.launch(k, None, sk)
        if self._macro_links:
            q.record(ev['macro'], sk)
            self._program_pack(q, it, ev['macro'], group, kind='macro')
            if group is None:
                self._program_macro_back(q, it)

    def _program_macro_back(self, q, it):
        """Unpack the neighbours' values into the ghost nodes; the sweep waits for it."""
        if not self._macro_links or self._nnx_serial(getattr(self, '_group', None)):
            return
        prof, timed = self._profile, not q.planned
        ev, sh = self._pev[it & 1], self._data_stream
        if timed:
            prof.record_gpu_start(TimeProfile.MACRO_DISTRIB, sh)
        for nid in sorted(self._macro_links):
            for k in self._macro_links[nid].unpacks[it & 1]:
                q.launch(k, None, sh)
        if timed:
            prof.record_gpu_end(TimeProfile.MACRO_DISTRIB, sh)
        q.record(ev['macro_halo'], sh)
        q.wait(self._calc_stream, ev['macro_halo'])

    def _program_front(self, q, it, sync_req, group=None):
        """The sweeps of every lattice over the whole subdomain (no face layers split off: the force reads the fields of
        the step, which the macro pass has just written) -> ghost-layer PBC kernels -> pack."""
        if self._nnx_serial(group):
            for k in self._sweep_kernels(it, sync_req):
                q.launch(k, None, self._calc_stream)
            return
        self._program_sweep_rest(q, it, self._sweep_kernels(it, sync_req), None, None, group)

    def _program_back(self, q, it):
        if self._nnx_serial(getattr(self, '_group', None)):
            return
        SubdomainRunner._program_back(self, q, it)


class IBMSubdomainRunner(SubdomainRunner):
    """Runner of lb_single.LBIBMFluidSim (reference subdomain_runner.py:1779-1837, which allocates the marker arrays and
    never uploads them): uploads the markers, allocates the zero acceleration field and the int64 accumulator, and puts
    the marker launches on the calc stream around the step's program -- spread and gather in front of it, clear-and-advect
    behind it (sailfish_amd/ibm.py).  They are direct entry points of the C ABI, which a step plan has no
    entry for, so they go around StepPlans.run: the same calls on the same stream whether the program between them is
    replayed from a plan or performed entry by entry.  The sweep always stores rho and v (the markers read v after every
    step, as the reference's force_field branch does), and steps are never replayed as graphs."""
    _markers = None

    def set_topology(self, all_specs, global_size, periodic):
        if len(all_specs) > 1:
            raise NotImplementedError('LBIBMFluidSim: more than one subdomain is not supported -- markers would cross the '
                                      'seams and there is no exchange of markers (%d subdomains)' % len(all_specs))
        super(IBMSubdomainRunner, self).set_topology(all_specs, global_size, periodic)

    def _init_accel_field(self, alloc):
        super(IBMSubdomainRunner, self)._init_accel_field(alloc)            # the zero field, handed to the module
        sim = self._sim
        if not sim.num_particles:
            return
        from sailfish_amd import ibm
        self._markers = ibm.Markers(self.backend, self.module, self.float, self.dim, self._spec.location,
                                    [p.position for p in sim._particles], [p.ref_position for p in sim._particles],
                                    [p.stiffness for p in sim._particles])
        sim.particle_positions = np.array(self._markers.position.T)

    def _sweep_kernels(self, it, sync_req):
        kernels = self._kernels_full
        return kernels.primary if (it & 1) == 0 else kernels.secondary

    def step(self, sync_req=False):
        m = self._markers
        if m is not None:
            m.front(self._calc_stream)
        super(IBMSubdomainRunner, self).step(True)
        if m is not None:
            gpu_map = 0 if int(self._desc.fluid_only) else self.gpu_geo_map()
            m.back(gpu_map, self.gpu_field(self._sim.v), self._calc_stream)

    def fast_forward(self):
        return 0

    def particle_positions(self):
        """[n, dim] positions of the markers as they are after the last enqueued step, copied back from the device."""
        if self._markers is None:
            return np.zeros((0, self.dim), dtype=self.float)
        return self._markers.positions(self._calc_stream)

    @property
    def ibm_outside(self):
        """Markers the last step held in place: a node of their stencil is not a real node of the subdomain."""
        return 0 if self._markers is None else self._markers.outside_count(self._calc_stream)

    def _fields_to_host(self, sync=True):
        super(IBMSubdomainRunner, self)._fields_to_host(sync)
        if self._markers is not None:
            self._sim.particle_positions = self.particle_positions()

    def save_checkpoint(self):
        if self._markers is not None:
            self._sim.particle_positions = self.particle_positions()
        super(IBMSubdomainRunner, self).save_checkpoint()

    def restore_checkpoint(self, fname):
        super(IBMSubdomainRunner, self).restore_checkpoint(fname)
        if self._markers is not None and self._sim.particle_positions is not None:
            self._markers.set_positions(self._sim.particle_positions)


class ThermalSubdomainRunner(SubdomainRunner):
    """Runner of lb_thermal.LBThermalFluidSim: allocates the zero acceleration field and the two copies of
    the temperature lattice, puts the init launch behind the flow's SetInitialConditions and the thermal launch on the calc
    stream behind every step's program (sailfish_amd/thermal.py).  They are direct entry points of the C ABI, which a step
    plan has no entry for, so they go around StepPlans.run: the same calls on the same stream whether the program in front
    of them is replayed from a plan or performed entry by entry.  The sweep always stores rho and v (the temperature
    collides with the v of every step), and steps are never replayed as graphs."""
    _thermal = None

    def set_topology(self, all_specs, global_size, periodic):
        if len(all_specs) > 1:
            raise NotImplementedError('LBThermalFluidSim: more than one subdomain is not supported -- the temperature '
                                      'populations would have to be exchanged across the seams (%d subdomains)' % len(all_specs))
        super(ThermalSubdomainRunner, self).set_topology(all_specs, global_size, periodic)

    def _init_accel_field(self, alloc):
        super(ThermalSubdomainRunner, self)._init_accel_field(alloc)        # the zero field, handed to the module
        from sailfish_amd import thermal
        sim = self._sim
        self._thermal = thermal.ThermalLattice(self.backend, self.module, self.float, self.dim, self._physical_size,
                                               self._local_periodic(), sim.thermal_diffusivity, sim.t_ref, sim.buoyancy)

    def _thermal_map(self):
        return 0 if int(self._desc.fluid_only) else self.gpu_geo_map()

    def _gpu_initial_conditions(self):
        super(ThermalSubdomainRunner, self)._gpu_initial_conditions()
        sim = self._sim
        if int(self._desc.fluid_only) and np.isfinite(sim.wall_temperature).any():
            raise ValueError('LBThermalFluidSim: wall_temperature is finite at %d nodes of a subdomain without walls or boundary '
                             'nodes: its kernels run without the node map and never read a wet node\'s own entry, so the '
                             'temperatures would be ignored' % int(np.isfinite(sim.wall_temperature).sum()))
        self._thermal.init(self._thermal_map(), self.gpu_field(sim.T), self.gpu_field(sim.v), self._calc_stream)

    def _sweep_kernels(self, it, sync_req):
        kernels = self._kernels_full
        return kernels.primary if (it & 1) == 0 else kernels.secondary

    def step(self, sync_req=False):
        sim = self._sim
        it = sim.iteration
        super(ThermalSubdomainRunner, self).step(True)
        self._thermal.back(it, self._thermal_map(), self.gpu_field(sim.v), self.gpu_field(sim.wall_temperature),
                           self.gpu_field(sim.T), self._calc_stream)

    def fast_forward(self):
        return 0

    def thermal_populations(self, copy=None):
        """Copy `copy` of the temperature populations (default: the one the next step reads), [Q] + the padded array shape."""
        if copy is None:
            copy = self._sim.iteration & 1
        return self._thermal.populations(copy, self._calc_stream)

    def release(self):
        self._thermal = None            # (the device copies go with every buffer of the backend; this drops the host mirrors)
        super(ThermalSubdomainRunner, self).release()

    def save_checkpoint(self):
        # what the next step reads and no prepare() can form again: the source copy of the populations and the field
        self._sim.thermal_g = self.thermal_populations()
        self.backend.from_buf(self._gpu_accel_field)
        self._sim.thermal_field = np.array(self._host_accel_field)
        super(ThermalSubdomainRunner, self).save_checkpoint()

    def restore_checkpoint(self, fname):
        super(ThermalSubdomainRunner, self).restore_checkpoint(fname)
        sim = self._sim
        if sim.thermal_g is not None:
            self._thermal.set_populations(sim.iteration & 1, sim.thermal_g)
            self._host_accel_field[...] = sim.thermal_field
            self.backend.to_buf(self._gpu_accel_field)
