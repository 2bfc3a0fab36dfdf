"""Single-subdomain driver on top of the backend interface.

A thin, allocation-owning helper used by bench.py, __graft_entry__.smoke() and
the GPU parity tests: it performs exactly the sequence of backend calls the
subdomain runner's step() performs for one subdomain without neighbours
(reference sailfish/subdomain_runner.py:960-1009: CollideAndPropagate, then
ApplyPeriodicBoundaryConditions per periodic axis, A/B swap or AA parity), but
takes plain numpy inputs instead of the LBSim/Subdomain classes.
"""
import os

import numpy as np

from sailfish_amd import hipabi, placement, sym


def padded_nx(lat_nx, alignment=32):
    """x padding, reference subdomain_runner.py:367-373 (--mem_alignment, default 32 nodes)."""
    return int(np.ceil(float(lat_nx) / alignment)) * alignment


def make_box_desc(grid, size, model='bgk', precision='single', access_pattern='AA', visc=1.0 / 6.0,
                  periodic_fused=(0, 0, 0), fluid_only=True, accel=None, incompressible=False,
                  relaxation_enabled=True, type_kind=None, node_params=None, nt_bits=None, use_link_tags=True,
                  alignment=32, dist_pad=None, regularized=False, subgrid=None, smagorinsky_const=0.1,
                  entropic_equilibrium=False, entropy_tolerance=0.0, alpha_tolerance=1e-10, accel_field=False):
    """size = (nx, ny[, nz]) real nodes; a ghost envelope of 1 is added.  accel_field: the module reads an acceleration
    per node (BoxSim(accel_field=...) hands it over); `accel` stays the uniform part."""
    dim = grid.dim
    assert len(size) == dim
    lat = [s + 2 for s in size]
    kw = dict(lattice=grid.slf_id,
              model=hipabi.SLF_MRT if model == 'mrt' else hipabi.SLF_BGK,
              precision=4 if precision == 'single' else 8,
              access_pattern=hipabi.SLF_AA if access_pattern == 'AA' else hipabi.SLF_AB,
              lat_nx=lat[0], lat_ny=lat[1], lat_nz=lat[2] if dim == 3 else 1,
              arr_nx=padded_nx(lat[0], alignment),
              arr_ny=lat[1], arr_nz=lat[2] if dim == 3 else 1,
              periodic_fused=list(periodic_fused), fluid_only=int(fluid_only),
              tau=sym.relaxation_time(visc), visc=visc, mrt_rates=sym.mrt_rates(grid, visc),
              incompressible=int(incompressible), relaxation_enabled=int(relaxation_enabled),
              use_link_tags=int(use_link_tags))
    if accel is not None:
        kw['has_force'] = 1
        kw['accel'] = list(accel) + [0.0] * (3 - len(accel))
    if accel_field:
        kw['accel_field'] = 1
        kw['has_force'] = 1
    if type_kind is not None:
        kw['type_kind'] = type_kind
    if node_params is not None:
        kw['node_params'] = node_params
    if nt_bits is not None:
        misc, param, scratch = nt_bits
        kw.update(nt_type_mask=(1 << misc) - 1, nt_misc_shift=misc, nt_param_shift=param, nt_scratch_shift=scratch)
    if dist_pad:
        kw['dist_stride'] = kw['arr_nx'] * kw['arr_ny'] * kw['arr_nz'] + int(dist_pad)
    if regularized or subgrid:
        kw.update(regularized=int(bool(regularized)), smagorinsky_const=float(smagorinsky_const),
                  subgrid=hipabi.SLF_SUBGRID_LES_SMAGORINSKY if subgrid else hipabi.SLF_SUBGRID_NONE)
    if model == 'elbm':
        from sailfish_amd.lb_single import LBFluidSim
        kw.update(LBFluidSim.elbm_desc(grid, visc, precision, entropic_equilibrium, entropy_tolerance, alpha_tolerance))
    elif entropic_equilibrium:
        kw['entropic_equilibrium'] = 1        # (refused by the library: it belongs to model = elbm)
    return hipabi.make_desc(**kw)


class BoxSim(object):
    """One subdomain, no neighbours, on one GPU through the backend interface."""

    def __init__(self, backend, desc, periodic=(False, False, False), node_map=None, tune_placement=False,
                 alpha_field=None, accel_field=None, accel_field_fill=0.0):
        """accel_field (modules built with accel_field): the acceleration at the real nodes, [dim, (nz,) ny, nx]; the ghost
        and padding entries of the uploaded array hold accel_field_fill (no sweep reads them).
        alpha_field (entropic modules): True = the alpha array exists (filled with 2) and is the trailing argument of
        CollideAndPropagate; None = as the module's model says; False = no array (every Newton iteration starts from 2)."""
        self.backend = backend
        self.desc = desc
        grid = [g for g in sym.KNOWN_GRIDS if g.slf_id == desc.lattice][0]
        self.dim, self.Q = grid.dim, grid.Q
        self.dtype = np.float32 if desc.precision == 4 else np.float64
        self.shape = (desc.arr_nz, desc.arr_ny, desc.arr_nx)
        self.nodes = desc.arr_nz * desc.arr_ny * desc.arr_nx
        self.aa = desc.access_pattern == hipabi.SLF_AA
        # axes that need ghost-layer PBC kernels = periodic and not wrapped by the sweep
        self.pbc_axes = [a for a in range(self.dim) if periodic[a] and not desc.periodic_fused[a]]
        self.iteration = 0
        for a in range(self.dim):
            desc.periodic_local[a] = int(bool(periodic[a]))
        b = backend
        self.stride = hipabi.dist_stride(desc)
        fbytes = self.stride * self.dtype().itemsize
        self.module = b.build(desc)
        off = b.dist_align_offset(self.dtype().itemsize)
        # large distribution arrays are *placed*: spread over physical HBM (placement.py)
        self.placed = []
        self.placement_info = None
        self.placement_tuning = None
        if placement.enabled() and self.Q * fbytes >= placement.MIN_BYTES and not int(desc.node_addressing):
            sizes = [self.Q * fbytes] * (1 if self.aa else 2)
            if tune_placement and os.environ.get('SLF_PLACEMENT_TUNE', '1') != '0' and not placement.holding_now():
                # placement by measurement (placement.choose): what SubdomainRunner does for its arrays
                probe_stream = b.make_stream()
                self.placed, self.placement_tuning = placement.choose(
                    lambda: b.alloc_placed(sizes, off),
                    lambda bs: placement.probe_sweep(b, desc, self.dim, bs[0].addr, bs[-1].addr, self.Q * fbytes, probe_stream),
                    lambda bs: [b.free_buf(pb.addr) for pb in bs], room=lambda: placement.room_for(b, sum(sizes)))
            else:
                self.placed = b.alloc_placed(sizes, off)
            self.placement_info = b.last_placement
            self.gpu_dist = [pb.addr for pb in self.placed]
        else:
            self.gpu_dist = [b.alloc_buf(size=self.Q * fbytes, align_offset=off)]
            if not self.aa:
                self.gpu_dist.append(b.alloc_buf(size=self.Q * fbytes, align_offset=off))
        # host mirrors of the macroscopic fields (ghost = +inf sentinel, reference
        # subdomain_runner.py:278-297)
        self.rho = np.full(self.shape, np.inf, dtype=self.dtype)
        self.v = [np.full(self.shape, np.inf, dtype=self.dtype) for _ in range(self.dim)]
        foff = b.dist_align_offset(self.dtype().itemsize)      # x = 1 of every field row on a 128-byte line as well
        self.gpu_rho = b.alloc_buf(like=self.rho, align_offset=foff)
        self.gpu_v = [b.alloc_buf(like=a, align_offset=foff) for a in self.v]
        self.alpha = self.gpu_alpha = None
        if alpha_field or (alpha_field is None and desc.model == hipabi.SLF_ELBM):
            self.alpha = np.full(self.shape, 2.0, dtype=self.dtype)
            self.gpu_alpha = b.alloc_buf(like=self.alpha, align_offset=foff)
        self.accel_field = self.gpu_accel_field = None
        if accel_field is not None:
            self.accel_field = np.full((self.dim,) + self.shape, accel_field_fill, dtype=self.dtype)
            for d in range(self.dim):
                self.real_view(self.accel_field[d])[...] = np.asarray(accel_field[d], dtype=np.float64)
            self.gpu_accel_field = b.alloc_buf(like=self.accel_field, align_offset=foff)
            b.set_accel_field(self.module, self.gpu_accel_field)
        self.gpu_map = 0
        self.node_map = None
        if node_map is not None:
            self.node_map = np.ascontiguousarray(node_map, dtype=np.uint32).reshape(self.shape)
            self.gpu_map = b.alloc_buf(like=self.node_map, align_offset=b.dist_align_offset(4))
        self.stream = b.make_stream()
        self.row_classes = None
        if self.gpu_map and b.supports_row_classes(desc) and os.environ.get('SLF_ROW_CLASSES', '1') != '0':
            self.row_classes = b.classify_rows(self.module, self.gpu_map, self.stream)
        self._make_kernels()

    def real_view(self, arr):
        d = self.desc
        if self.dim == 3:
            return arr[..., 1:d.lat_nz - 1, 1:d.lat_ny - 1, 1:d.lat_nx - 1]
        return arr[..., 0, 1:d.lat_ny - 1, 1:d.lat_nx - 1]

    def _make_kernels(self):
        b, m = self.backend, self.module
        sig = 'P' * (4 + self.dim) + 'i'
        self.k_sweep = {}
        for save in (0, 1):
            ks = []
            pairs = [(0, 0)] if self.aa else [(0, 1), (1, 0)]
            for i, o in pairs:
                args = [self.gpu_map, self.gpu_dist[i], self.gpu_dist[o], self.gpu_rho] + self.gpu_v + [save]
                csig = sig
                if self.gpu_alpha is not None:
                    args.append(self.gpu_alpha)
                    csig += 'P'
                ks.append(b.get_kernel(m, 'CollideAndPropagate', (64,), args, csig, needs_iteration=self.aa))
            self.k_sweep[save] = ks
        self._make_pair_kernels(sig)
        self.k_init = []
        for dbuf in self.gpu_dist:
            args = [dbuf] + self.gpu_v + [self.gpu_rho, self.gpu_map]
            self.k_init.append(b.get_kernel(m, 'SetInitialConditions', (64,), args, 'P' * (3 + self.dim)))
        self.k_pbc = {}
        for i, dbuf in enumerate(self.gpu_dist):
            for axis in self.pbc_axes:
                self.k_pbc[(i, axis, False)] = b.get_kernel(m, 'ApplyPeriodicBoundaryConditions', (64,),
                                                            [dbuf, axis], 'Pi')
                if self.aa:
                    self.k_pbc[(i, axis, True)] = b.get_kernel(m, 'ApplyPeriodicBoundaryConditionsWithSwap',
                                                               (64,), [dbuf, axis], 'Pi')
        args = [self.gpu_map, self.gpu_dist[0], self.gpu_dist[0], self.gpu_rho] + self.gpu_v + [1]
        self.k_macro = b.get_kernel(m, 'ComputeMacroFields', (64,), args, sig, needs_iteration=self.aa)

    def _make_pair_kernels(self, sig):
        """The two kernel objects that advance TWO steps per launch (copy 0 -> 1, 1 -> 0; C ABI slf_kernel_set_pair), where
        the library accepts them: two-copy D3Q19 / f32 / BGK boxes wrapped in-sweep on every axis.
        SLF_STEP_PAIRS=0 switches pairing off; SLF_PAIR_ROWS / SLF_PAIR_ZCHUNK size the piece of the box a workgroup
        takes (0 / unset: the library's default).  A slab with a halo never pairs: its face layers leave every step."""
        b = self.backend
        self.k_pair = None          # [kernel that reads gpu_dist[0], kernel that reads gpu_dist[1]]
        self.pair_refused = None    # the library's reason where it does not accept
        self.pair_launches = 0
        self._pending = False       # one step counted in `iteration` and not enqueued yet
        self._flipped = False       # an odd number of pair launches since the arrays last held what single steps leave
        if self.aa or getattr(self, 'halo', False) or not hasattr(b, 'set_kernel_pair'):
            return
        if os.environ.get('SLF_STEP_PAIRS', '1') == '0':
            self.pair_refused = 'SLF_STEP_PAIRS=0'
            return
        if self.pbc_axes or self.gpu_alpha is not None:
            self.pair_refused = 'pair sweep: every axis must be wrapped inside the sweep'
            return
        rows = int(os.environ.get('SLF_PAIR_ROWS', '0') or 0)
        zchunk = int(os.environ.get('SLF_PAIR_ZCHUNK', '0') or 0)
        ks = []
        for i, o in ((0, 1), (1, 0)):
            args = [self.gpu_map, self.gpu_dist[i], self.gpu_dist[o], self.gpu_rho] + self.gpu_v + [0]
            k = b.get_kernel(self.module, 'CollideAndPropagate', (64,), args, sig)
            why = b.set_kernel_pair(k, rows, zchunk)
            if why is not None:
                self.pair_refused = why
                return
            ks.append(k)
        self.k_pair = ks

    def _flush(self):
        """Brings the device to what `iteration` says, in the array single steps would have left it in: enqueues the
        pending step with the single-step kernel and, after an odd number of pair launches (the populations sit in the
        other array), copies them over and puts `gpu_dist` and the kernel lists back in their original order.  Everything
        that looks at or replaces device state calls this first."""
        if getattr(self, 'k_pair', None) is None:
            return
        b = self.backend
        if self._pending:
            self._pending = False
            b.run_kernel(self.k_sweep[0][(self.iteration - 1) & 1], None, self.stream)
        if self._flipped:
            cur = self.gpu_dist[self.iteration & 1]
            other = self.gpu_dist[1 - (self.iteration & 1)]
            b.copy_dist_async(other, cur, self.Q * self.stride * self.dtype().itemsize, self.stream)
            self._flip()

    def _flip(self):
        """`gpu_dist[iteration & 1]` is the current copy, and kernel i of a list reads gpu_dist[i]: after a pair launch the
        populations are in the other physical array while the parity of `iteration` is what it was, so the lists turn
        round, in place (whoever holds the list sees it)."""
        self.gpu_dist.reverse()
        self.k_pair.reverse()
        for ks in self.k_sweep.values():
            ks.reverse()
        self._flipped = not self._flipped

    def set_fields(self, rho, v):
        """rho, v[d]: arrays over the *real* nodes ((nz,) ny, nx)."""
        self.real_view(self.rho)[...] = rho
        for d in range(self.dim):
            self.real_view(self.v[d])[...] = v[d]
        self.backend.to_buf(self.gpu_rho)
        for g in self.gpu_v:
            self.backend.to_buf(g)

    def initial_conditions(self):
        """SetInitialConditions on every dist copy (reference lb_single.py:72-94)."""
        self._flush()
        for k in self.k_init:
            self.backend.run_kernel(k, None, self.stream)
        self.iteration = 0
        self.backend.set_iteration(0)

    def _sweep_of(self, it, save_macro):
        """(sweep kernel, copy of the arrays it writes, does it leave the populations in opposite slots) of step `it`:
        in place one kernel and one copy, the even steps swap; two copies: the kernel and the copy alternate."""
        ks = self.k_sweep[int(save_macro)]
        if self.aa:
            return ks[0], 0, (it & 1) == 0
        return ks[it & 1], 1 - (it & 1), False

    def step(self, save_macro=False, region=None):
        b = self.backend
        if self.k_pair is not None:
            if not save_macro and region is None:
                # deferred stepping: the first of two steps is only counted, the second enqueues both as one launch
                if self._pending:
                    b.run_kernel(self.k_pair[(self.iteration - 1) & 1], None, self.stream)
                    self.pair_launches += 1
                    self._flip()
                self._pending = not self._pending
                self.iteration += 1
                b.set_iteration(self.iteration)
                return
            if self._pending:       # (the arrays may stay turned round: this step's kernels come from the same lists)
                self._pending = False
                b.run_kernel(self.k_sweep[0][(self.iteration - 1) & 1], None, self.stream)
        k, out, swap = self._sweep_of(self.iteration, save_macro)
        b.run_kernel(k, region, self.stream)
        for axis in self.pbc_axes:
            b.run_kernel(self.k_pbc[(out, axis, swap)], None, self.stream)
        self.iteration += 1
        b.set_iteration(self.iteration)

    def run(self, n, save_last=True):
        for i in range(n):
            self.step(save_macro=(save_last and i == n - 1))

    def sync(self):
        self._flush()
        self.stream.synchronize()

    def release(self):
        """Frees the device memory of this simulation."""
        self.sync()
        b = self.backend
        for addr in list(self.gpu_dist) + [self.gpu_rho] + list(self.gpu_v) + ([self.gpu_map] if self.gpu_map else []) + \
                ([self.gpu_alpha] if self.gpu_alpha is not None else []) + \
                ([self.gpu_accel_field] if self.gpu_accel_field is not None else []):
            b.free_buf(addr)
        self.gpu_dist = []
        # drop the kernel objects: the backend's registry of iteration-dependent kernels holds them weakly
        for name in ('k_init', 'k_sweep', 'k_pair', 'k_pbc', 'k_macro', 'k_halo'):
            if hasattr(self, name):
                setattr(self, name, None)

    def fetch_fields(self):
        self.sync()       # (flushes a pending step)
        self.backend.from_buf(self.gpu_rho)
        for g in self.gpu_v:
            self.backend.from_buf(g)
        return self.rho, self.v

    def fetch_alpha(self):
        self.sync()
        self.backend.from_buf(self.gpu_alpha)
        return self.alpha

    def set_alpha(self, alpha):
        """alpha over the real nodes (or a scalar)."""
        self.real_view(self.alpha)[...] = alpha
        self.backend.to_buf(self.gpu_alpha)

    def current_dist_index(self):
        return 0 if self.aa else (self.iteration & 1)

    def get_dist(self, which=None):
        """Raw distributions [Q, (nz,) ny, arr_nx] (reference _debug_get_dist, subdomain_runner.py:1363-1381)."""
        self.sync()
        idx = self.current_dist_index() if which is None else which
        raw = np.zeros((self.Q, self.stride), dtype=self.dtype)
        self.backend.from_buf(self.gpu_dist[idx], raw)
        return np.ascontiguousarray(raw[:, :self.nodes]).reshape((self.Q,) + self.shape)

    def set_dist(self, host, which=None):
        self._flush()
        idx = self.current_dist_index() if which is None else which
        raw = np.zeros((self.Q, self.stride), dtype=self.dtype)
        raw[:, :self.nodes] = np.asarray(host, dtype=self.dtype).reshape(self.Q, self.nodes)
        self.backend.to_buf(self.gpu_dist[idx], raw)
