"""numpy twin of one time step of a single-fluid BGK module, with the lattice taken from tables (sailfish_amd.sym): what
csrc/slf_lat.hip computes on D3Q15 / D3Q27, and -- with the tables of D3Q19 -- what the CPU oracle computes, bit for bit
(tests/test_lat_twin.py carries the oracle's pinned arithmetic over that way; what then differs for the other lattices is
tables, which tests/golden/lattices_q15_q27.json and the arith_lat_* fixtures pin).

Every floating-point operation is one numpy operation in the module's format, in the order written at the top of
csrc/slf_lat.hip; there is no fused multiply-add and no transcendental function in a step, so the kernels (built with
-ffp-contract=off) have nothing to round differently.

TwinSim has the interface of oracle.OracleSim (new_dist, init, step, pbc, sparse) and works on the same arrays: populations
[Q, arr_nz, arr_ny, arr_nx] inside a buffer with the descriptor's direction stride, ghost layer included.  TwinGroup steps
the subdomains of a decomposition in lock-step and exchanges their halos through the index lists of
sailfish_amd.subdomain_connection, like tests/_oracle_group.OracleGroup.  Test-only."""
import numpy as np

from sailfish_amd import hipabi, subdomain_connection, sym

PROP_AB, PROP_AA_EVEN, PROP_AA_ODD = 0, 1, 2
EXCLUDED = (hipabi.SLF_NK_GHOST, hipabi.SLF_NK_UNUSED, hipabi.SLF_NK_PROPAGATION_ONLY)
WET = (hipabi.SLF_NK_FLUID, hipabi.SLF_NK_HALF_BB)


def grid_of(desc):
    return [g for g in sym.KNOWN_GRIDS if g.slf_id == desc.lattice][0]


# ---- the arithmetic of a node (arrays of nodes; f: [Q, n]) --------------------------------------------------------------

def weights(grid, R):
    """w_i as the kernels hold them: the double quotient, rounded once to the format."""
    return [R(float(w.numerator) / float(w.denominator)) for w in grid.weights]


def density(f):
    rho = f[0].copy()
    for i in range(1, len(f)):
        rho = rho + f[i]
    return rho


def momentum(grid, f, d, R):
    acc = np.zeros_like(f[0])
    for i in range(1, grid.Q):
        e = grid.basis[i][d]
        if e > 0:
            acc = acc + f[i]
        elif e < 0:
            acc = acc - f[i]
    return acc


def macro(grid, f, incompressible, R):
    rho = density(f)
    v = [momentum(grid, f, d, R) for d in range(grid.dim)]
    if not incompressible:
        v = [c / rho for c in v]
    return rho, v


def usq15(v, R):
    s = v[0] * v[0] + v[1] * v[1]
    if len(v) == 3:
        s = s + v[2] * v[2]
    return R(1.5) * s


def edot(grid, i, v, like):
    """e_i . v, components in x, y, z order, +-1 as add / subtract; v: arrays or scalars of the format."""
    acc = np.zeros_like(like)
    for d in range(grid.dim):
        e = grid.basis[i][d]
        if e > 0:
            acc = acc + v[d]
        elif e < 0:
            acc = acc - v[d]
    return acc


def feq(grid, i, rho, rho0, v, u15, R, w):
    if not any(grid.basis[i]):
        return w[i] * (rho + rho0 * (R(0) - u15))
    eu = edot(grid, i, v, rho)
    return w[i] * (rho + rho0 * (eu * (R(3) + R(4.5) * eu) - u15))


def relax(grid, f, rho, v, omega, guo_pref, incompressible, accel, edm, R):
    """bgk_relax_accel (csrc/slf_node.h): returns the post-collision populations and the velocity the sweep stores.
    accel: None (no body force) or dim values of the format."""
    w = weights(grid, R)
    rho0 = np.ones_like(rho) if incompressible else rho
    Q = grid.Q
    out = [None] * Q
    if accel is not None and edm:
        vs = [c + a for c, a in zip(v, accel)]
        u15, u15s = usq15(v, R), usq15(vs, R)
        for i in range(Q):
            fe = feq(grid, i, rho, rho0, v, u15, R, w)
            fs = feq(grid, i, rho, rho0, vs, u15s, R, w)
            t = f[i] + omega * (fe - f[i])
            out[i] = t + (fs - fe)
        return np.stack(out), [c + R(0.5) * a for c, a in zip(v, accel)]
    if accel is not None:
        v = [c + R(0.5) * a for c, a in zip(v, accel)]
    u15 = usq15(v, R)
    for i in range(Q):
        fe = feq(grid, i, rho, rho0, v, u15, R, w)
        out[i] = f[i] + omega * (fe - f[i])
    if accel is not None:
        pref = rho * guo_pref
        va = v[0] * accel[0] + v[1] * accel[1]
        if grid.dim == 3:
            va = va + v[2] * accel[2]
        for i in range(Q):
            eu = edot(grid, i, v, rho)
            ea = edot(grid, i, accel, R(0))
            t = (ea - va) + R(3) * eu * ea
            out[i] = out[i] + pref * w[i] * t
    return np.stack(out), v


def guo_term(grid, rho, v, accel, guo_pref, R):
    """The Guo forcing term alone (for the fixtures): (rho pref) w_i (((e_i.a) - (v.a)) + 3 (e_i.v) (e_i.a)), v as given."""
    w = weights(grid, R)
    pref = rho * guo_pref
    va = v[0] * accel[0] + v[1] * accel[1]
    if grid.dim == 3:
        va = va + v[2] * accel[2]
    out = []
    for i in range(grid.Q):
        eu = edot(grid, i, v, rho)
        ea = edot(grid, i, accel, rho)
        out.append(pref * w[i] * ((ea - va) + R(3) * eu * ea))
    return np.stack(out)


def equilibrium(grid, rho, v, incompressible, R):
    w = weights(grid, R)
    rho0 = np.ones_like(rho) if incompressible else rho
    u15 = usq15(v, R)
    return np.stack([feq(grid, i, rho, rho0, v, u15, R, w) for i in range(grid.Q)])


# ---- a subdomain ----------------------------------------------------------------------------------------------------------

class TwinSim(object):
    """One subdomain of a single-fluid BGK module described by a hipabi.SlfModuleDesc; direct addressing; node kinds
    fluid, ghost, unused, propagation-only, full-way and half-way bounce-back."""

    def __init__(self, desc, grid=None):
        self.desc = d = desc
        self.grid = grid or grid_of(desc)
        assert d.model == hipabi.SLF_BGK and not int(d.node_addressing) and not int(d.simtype)
        self.Q, self.dim = self.grid.Q, self.grid.dim
        assert self.dim == 3
        self.dtype = self.R = np.float32 if d.precision == 4 else np.float64
        self.shape = (d.arr_nz, d.arr_ny, d.arr_nx)
        self.lat = (d.lat_nz, d.lat_ny, d.lat_nx)
        self.n = d.arr_nz * d.arr_ny * d.arr_nx
        self.stride = hipabi.dist_stride(d)
        self.opp = self.grid.idx_opposite
        z, y, x = np.meshgrid(*[np.arange(1, n - 1) for n in self.lat], indexing='ij')
        self.zyx = [z.ravel(), y.ravel(), x.ravel()]

    def new_dist(self):
        raw = np.full((self.Q, self.stride), np.nan, dtype=self.dtype)
        return raw[:, :self.n].reshape((self.Q,) + self.shape)

    def new_field(self, fill=0.0):
        return np.full(self.shape, fill, dtype=self.dtype)

    def init(self, dist, rho, vx, vy, vz):
        """SetInitialConditions: the equilibrium of the host fields on every node of the lattice box (ghosts carry the
        fields' non-finite sentinels)."""
        R = self.R
        sl = tuple(slice(0, n) for n in self.lat)
        with np.errstate(all='ignore'):
            fe = equilibrium(self.grid, rho[sl].astype(R), [c[sl].astype(R) for c in (vx, vy, vz)],
                             int(self.desc.incompressible) != 0, R)
        dist[(slice(None),) + sl] = fe

    def _neighbour(self, sign):
        """Coordinates of node + sign * e_i for every real node and direction, wrapped along the axes the sweep wraps."""
        d = self.desc
        out = []
        for i in range(self.Q):
            e = self.grid.basis[i]
            c = []
            for k, axis in enumerate((2, 1, 0)):       # arrays are z, y, x; basis vectors x, y, z
                s = sign * e[axis]
                t = self.zyx[k] + s
                if d.periodic_fused[axis] and s:
                    n = self.lat[k]
                    t = np.where(t == n - 1, 1, np.where(t == 0, n - 2, t))
                c.append(t)
            out.append(tuple(c))
        return out

    def step(self, prop, nmap, din, dout, rho, vx, vy, vz, options=0, region=None):
        assert region is None
        d, g, R, Q, opp = self.desc, self.grid, self.R, self.Q, self.opp
        z, y, x = self.zyx
        here = (z, y, x)
        if d.fluid_only:
            code = np.zeros(len(z), dtype=np.uint32)
            kind = np.full(len(z), hipabi.SLF_NK_FLUID)
        else:
            code = nmap[here]
            kind = np.array(list(d.type_kind[:d.n_types]))[code & np.uint32(d.nt_type_mask)]
        active = ~np.isin(kind, EXCLUDED)
        wet = np.isin(kind, WET) & active
        fwd, bwd = self._neighbour(+1), self._neighbour(-1)
        # 1. load
        if prop == PROP_AA_ODD:
            f = np.stack([din[(opp[i],) + bwd[i]] for i in range(Q)])
        else:
            f = np.stack([din[(i,) + here] for i in range(Q)])
        # 2. wet nodes
        omega = R(1.0 / d.tau)
        guo_pref = R(3.0 * (1.0 - 0.5 / d.tau))
        accel = [R(d.accel[k]) for k in range(3)] if d.has_force else None
        edm = int(d.force_implementation) == hipabi.SLF_FORCE_EDM
        inc = int(d.incompressible) != 0
        fw = f[:, wet]
        with np.errstate(all='ignore'):
            r, v = macro(g, fw, inc, R)
            if d.relaxation_enabled:
                fw, v = relax(g, fw, r, v, omega, guo_pref, inc, accel, edm, R)
        f[:, wet] = fw
        if options & 1:
            w = tuple(c[wet] for c in here)
            rho[w] = r
            for field, c in zip((vx, vy, vz), v):
                field[w] = c
        # 3. full-way walls
        bb = kind == hipabi.SLF_NK_FULL_BB
        f[:, bb] = f[opp][:, bb]
        # 4. half-way walls: f_i of every direction i that points at a non-fluid node, where the next step reads opp(i)
        hb = (kind == hipabi.SLF_NK_HALF_BB) & active
        if hb.any():
            orient_shift = d.nt_misc_shift + d.nt_param_shift + d.nt_scratch_shift
            orientation = code >> np.uint32(orient_shift)
            for i in range(1, Q):
                if d.use_link_tags:
                    missing = ((orientation >> np.uint32(i - 1)) & np.uint32(1)) == 0
                else:
                    dots = np.array([0] + [sum(a * b for a, b in zip(g.basis[opp[i]], g.basis[g.dir2vecidx[o]]))
                                           for o in range(1, 2 * self.dim + 1)] + [0] * 64)
                    missing = dots[np.minimum(orientation, 2 * self.dim + 1)] > 0
                m = hb & missing
                if not m.any():
                    continue
                if prop == PROP_AA_EVEN:
                    dout[(i,) + tuple(c[m] for c in fwd[i])] = f[i, m]
                else:
                    dout[(opp[i],) + tuple(c[m] for c in here)] = f[i, m]
        # 5. store
        for i in range(Q):
            if prop == PROP_AA_EVEN:
                dout[(opp[i],) + tuple(c[active] for c in here)] = f[i, active]
            else:
                dout[(i,) + tuple(c[active] for c in fwd[i])] = f[i, active]

    # ---- ghost-layer periodicity (pbc_kernel, csrc/slf_plain.h) ----
    @staticmethod
    def _push_ok(c, e, lat, mode, earlier):
        real = (c >= 1) & (c <= lat - 2)
        if mode == 2 or (mode == 1 and earlier):
            return real
        pushed = (c >= 2) if e > 0 else ((c <= lat - 3) if e < 0 else real)
        return pushed if mode == 1 else (real & pushed)

    @staticmethod
    def _pull_ok(c, e, lat, mode, earlier):
        if mode == 1 and earlier:
            return (c + e >= 1) & (c + e <= lat - 2)
        return (c >= 1) & (c <= lat - 2)

    def pbc(self, dist, axis, with_swap=False):
        d = self.desc
        lat = [d.lat_nx, d.lat_ny, d.lat_nz]
        mode = [2 if d.periodic_fused[a] else (1 if d.periodic_local[a] else 0) for a in range(3)]
        b_ax, c_ax = [a for a in range(3) if a != axis]
        b, c = np.meshgrid(np.arange(lat[b_ax]), np.arange(lat[c_ax]), indexing='ij')
        b, c = b.ravel(), c.ravel()
        n = lat[axis]
        ok_fn = self._pull_ok if with_swap else self._push_ok

        def index(layer, sel):
            coords = {axis: np.full(int(sel.sum()), layer), b_ax: b[sel], c_ax: c[sel]}
            return (coords[2], coords[1], coords[0])

        for i in range(1, self.Q):
            e = self.grid.basis[i]
            ea = e[axis]
            if ea == 0:
                continue
            sel = ok_fn(b, e[b_ax], lat[b_ax], mode[b_ax], b_ax < axis) & ok_fn(c, e[c_ax], lat[c_ax], mode[c_ax], c_ax < axis)
            if with_swap:
                src, dst, q = (n - 2 if ea > 0 else 1), (0 if ea > 0 else n - 1), self.opp[i]
            else:
                src, dst, q = (0 if ea < 0 else n - 1), (n - 2 if ea < 0 else 1), i
            val = dist[(q,) + index(src, sel)]
            fin = np.isfinite(val)
            di = index(dst, sel)
            dist[(q,) + tuple(k[fin] for k in di)] = val[fin]

    def sparse(self, collect, idx, raw, buf):
        idx = np.asarray(idx, dtype=np.int64)
        if collect:
            buf[:] = raw[idx]
        else:
            fin = np.isfinite(buf)
            raw[idx[fin]] = buf[fin]


def raw_of(dist):
    base = dist
    while base.base is not None:
        base = base.base
    return base.reshape(-1)


class TwinSubdomain(object):
    """A runner's subdomain on the twin: geometry, descriptor and halo lists from the host layer (as
    tests/_oracle_group.OracleSubdomain), the arithmetic from `sim_of(desc)` -- TwinSim, or oracle.OracleSim for D3Q19."""

    def __init__(self, runner, sim_of=TwinSim):
        r = self.runner = runner
        r._init_geometry()
        r._sim.init_fields(r)
        r._subdomain.init_fields(r._sim)
        self.desc = r._module_desc()
        self.o = sim_of(self.desc)
        self.aa = self.desc.access_pattern == hipabi.SLF_AA
        dt = self.o.dtype
        self.node_map = np.ascontiguousarray(r._subdomain._type_map_base, dtype=np.uint32).reshape(self.o.shape)
        self.rho = np.ascontiguousarray(r.field_base(r._sim.rho), dtype=dt).reshape(self.o.shape)
        self.v = [np.ascontiguousarray(r.field_base(c), dtype=dt).reshape(self.o.shape) for c in r._sim.v]
        self.dist = [self.o.new_dist()] + ([] if self.aa else [self.o.new_dist()])
        with np.errstate(all='ignore'):
            for d in self.dist:
                self.o.init(d, self.rho, self.v[0], self.v[1], self.v[2])
        local = r._local_periodic()
        self.pbc_axes = [a for a in range(3) if local[a] and not r._fused[a]]
        self.iteration = 0
        self.links = {}
        if len(r._all_specs) > 1:
            self.links = subdomain_connection.build_halo_links(
                r._spec, r._all_specs, r._global_size, r._global_periodic, r._sim.grid, list(reversed(r._physical_size)),
                hipabi.dist_stride(self.desc), fused=r._fused)

    def compute(self, save=False):
        it = self.iteration
        opts = 1 if save else 0
        if getattr(self.runner._sim, 'time_dependent_force', False):
            for i, a in enumerate(self.runner._sim.body_force_at(it)):
                self.desc.accel[i] = float(a)
        if self.aa:
            self.o.step(PROP_AA_ODD if (it & 1) else PROP_AA_EVEN, self.node_map, self.dist[0], self.dist[0], self.rho, *self.v,
                        options=opts)
            out, swap = 0, (it & 1) == 0
        else:
            self.o.step(PROP_AB, self.node_map, self.dist[it & 1], self.dist[1 - (it & 1)], self.rho, *self.v, options=opts)
            out, swap = 1 - (it & 1), False
        for axis in self.pbc_axes:
            self.o.pbc(self.dist[out], axis, swap)
        self.mode = 'pull' if (self.aa and (it & 1) == 0) else 'push'
        self.out = out
        self.iteration += 1
        sends = {}
        for nid, link in self.links.items():
            idx = getattr(link, self.mode + '_send')
            buf = np.zeros(len(idx), dtype=self.o.dtype)
            if len(idx):
                self.o.sparse(True, idx, raw_of(self.dist[out]), buf)
            sends[nid] = buf
        return sends

    def finish(self, recvs):
        for nid, buf in recvs.items():
            idx = getattr(self.links[nid], self.mode + '_recv')
            assert len(idx) == len(buf)
            if len(idx):
                self.o.sparse(False, idx, raw_of(self.dist[self.out]), np.ascontiguousarray(buf))

    def current(self):
        return self.dist[0] if self.aa else self.dist[self.iteration & 1]


class TwinGroup(object):
    """Every subdomain of a simulation in one process, in lock-step."""

    def __init__(self, sim_cls, geo, cfg_kw, sim_of=TwinSim):
        from tests import _host
        self.cfg, self.specs, runners = _host.build_runners(sim_cls, 3, geo, cfg_kw)
        self.subs = [TwinSubdomain(r, sim_of) for r in runners]

    def step(self, save=False):
        sends = [s.compute(save) for s in self.subs]
        for s in self.subs:
            s.finish(dict((nid, sends[nid][s.runner._spec.id]) for nid in s.links))

    def run(self, n, save_last=True):
        for i in range(n):
            self.step(save_last and i == n - 1)
        return self

    def merged(self, what):
        """'dist' | 'rho' | 'v0' .. | 'kind' on the global grid (real nodes)."""
        s0 = self.subs[0]
        gshape = tuple(reversed(s0.runner._global_size))
        lead = (s0.o.Q,) if what == 'dist' else ()
        out = np.zeros(lead + gshape, dtype=np.int64 if what == 'kind' else s0.o.dtype)
        for s in self.subs:
            sp = s.runner._spec
            sl = tuple(slice(o, o + n) for o, n in zip(reversed(sp.location), reversed(sp.size)))
            ng = (Ellipsis,) + tuple(sp._nonghost_slice)
            if what == 'dist':
                out[(slice(None),) + sl] = s.current()[ng]
            elif what == 'rho':
                out[sl] = s.rho[ng]
            elif what == 'kind':
                d = s.desc
                kinds = np.array(list(d.type_kind[:d.n_types]) or [0])
                out[sl] = 0 if d.fluid_only else kinds[s.node_map[ng] & np.uint32(d.nt_type_mask)]
            else:
                out[sl] = s.v[int(what[1:])][ng]
        return out
