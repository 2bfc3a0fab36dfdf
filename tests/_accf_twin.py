"""numpy twin of one time step of a single-fluid BGK module with a per-node acceleration (slf_module_desc::accel_field): what
the ACCF instantiations of the per-node sweep (csrc/slf_kernels.hip) compute on D2Q9 and D3Q19.

The arithmetic of a node is tests/_lat_twin's (macro, relax, equilibrium: arrays of nodes, one numpy operation per
floating-point operation, in the module's format); relax() takes arrays for the acceleration.  The acceleration of node gi
is cp.accel[d] + field[d][gi] -- one addition in the format -- where the module has a field, cp.accel[d] otherwise, so a
twin without a field is the constant-force step and tests/test_accf_twin.py holds it against the CPU oracle bit for bit.

AccfTwin has the interface of oracle.OracleSim (new_dist, new_field, init, step, pbc, sparse) and works on the same arrays;
SetInitialConditions, the ghost-layer periodicity and the index-list copies move data without arithmetic of their own
interest here and are the oracle's.  BGK with Guo forcing and the exact difference method; fluid, ghost, unused,
propagation-only, full-way and half-way bounce-back nodes; direct addressing.  AccfTwinBox is the step sequence of
sailfish_amd.box.BoxSim on the twin (as tests/_oracle_box.OracleBox is on the oracle).  Test-only."""
import numpy as np

from oracle.oracle import OracleSim
from sailfish_amd import hipabi
from tests import _lat_twin as lt
from tests._oracle_box import OracleBox

PROP_AB, PROP_AA_EVEN, PROP_AA_ODD = lt.PROP_AB, lt.PROP_AA_EVEN, lt.PROP_AA_ODD


class AccfTwin(object):
    def __init__(self, desc):
        self.desc = d = desc
        self.grid = lt.grid_of(desc)
        assert d.lattice in (hipabi.SLF_D2Q9, hipabi.SLF_D3Q19)
        assert d.model == hipabi.SLF_BGK and not int(d.node_addressing) and not int(d.simtype)
        self._oracle = OracleSim(desc)          # init, pbc, sparse: data movement
        self.Q, self.dim = self.grid.Q, self.grid.dim
        self.dtype = self.R = np.float32 if d.precision == 4 else np.float64
        self.shape = (d.arr_nz, d.arr_ny, d.arr_nx)
        self.lat = (d.lat_nz, d.lat_ny, d.lat_nx)
        self.n = d.arr_nz * d.arr_ny * d.arr_nx
        self.stride = hipabi.dist_stride(d)
        self.opp = self.grid.idx_opposite
        zr = np.arange(1, d.lat_nz - 1) if self.dim == 3 else np.arange(1)
        z, y, x = np.meshgrid(zr, np.arange(1, d.lat_ny - 1), np.arange(1, d.lat_nx - 1), indexing='ij')
        self.zyx = [z.ravel(), y.ravel(), x.ravel()]
        self.accel_field = None                  # [dim, arr_nz, arr_ny, arr_nx] in the module's format

    def set_accel_field(self, field):
        field = np.asarray(field)
        assert field.shape == (self.dim,) + self.shape and field.dtype == self.dtype
        self.accel_field = field

    def new_dist(self):
        return self._oracle.new_dist()

    def new_field(self, fill=0.0):
        return self._oracle.new_field(fill)

    def init(self, dist, rho, vx, vy, vz=None):
        self._oracle.init(dist, rho, vx, vy, vz)

    def pbc(self, dist, axis, with_swap=False):
        self._oracle.pbc(dist, axis, with_swap)

    def sparse(self, collect, idx, dist, buf):
        self._oracle.sparse(collect, idx, dist, buf)

    def _neighbour(self, sign):
        """Coordinates of node + sign * e_i for every real node and direction, wrapped along the axes the sweep wraps."""
        d = self.desc
        out = []
        for i in range(self.Q):
            e = tuple(self.grid.basis[i]) + (0,) * (3 - self.dim)
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

    def node_accel(self, where):
        """The acceleration of the nodes `where` (index arrays z, y, x): dim arrays of the format, or None without a force."""
        d, R = self.desc, self.R
        if not (d.has_force or d.accel_field):
            return None
        uniform = [R(d.accel[k]) for k in range(self.dim)]
        if not d.accel_field:
            return uniform
        assert self.accel_field is not None, 'accel_field module without a field'
        return [uniform[k] + self.accel_field[k][where] for k in range(self.dim)]

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
        assert np.isin(kind, lt.EXCLUDED + lt.WET + (hipabi.SLF_NK_FULL_BB,)).all()
        active = ~np.isin(kind, lt.EXCLUDED)
        wet = np.isin(kind, lt.WET) & active
        fwd, bwd = self._neighbour(+1), self._neighbour(-1)
        # 1. load
        if prop == PROP_AA_ODD:
            f = np.stack([din[(opp[i],) + bwd[i]] for i in range(Q)])
        else:
            f = np.stack([din[(i,) + here] for i in range(Q)])
        # 2. wet nodes
        omega = R(1.0 / d.tau)
        guo_pref = R(3.0 * (1.0 - 0.5 / d.tau))
        wet_at = tuple(c[wet] for c in here)
        accel = self.node_accel(wet_at)
        edm = int(d.force_implementation) == hipabi.SLF_FORCE_EDM
        inc = int(d.incompressible) != 0
        fw = f[:, wet]
        with np.errstate(all='ignore'):
            r, v = lt.macro(g, fw, inc, R)
            if d.relaxation_enabled:
                fw, v = lt.relax(g, fw, r, v, omega, guo_pref, inc, accel, edm, R)
        f[:, wet] = fw
        if options & 1:
            rho[wet_at] = r
            for field, c in zip((vx, vy, vz), v):
                field[wet_at] = c
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


class AccfTwinBox(OracleBox):
    """tests/_oracle_box.OracleBox with the twin in the oracle's place.  accel_field: the acceleration at the real nodes,
    [dim, (nz,) ny, nx] (the module must have been described with accel_field); ghost and padding entries hold `fill`."""

    def __init__(self, desc, periodic=(False, False, False), node_map=None, accel_field=None, fill=np.nan):
        super(AccfTwinBox, self).__init__(desc, periodic, node_map)
        self.o = AccfTwin(desc)
        self.accel_field = None
        if accel_field is not None:
            self.accel_field = np.full((self.dim,) + self.shape, fill, dtype=self.dtype)
            for k in range(self.dim):
                self.real_view(self.accel_field[k])[...] = np.asarray(accel_field[k], dtype=np.float64)
            self.o.set_accel_field(self.accel_field)


def linear_field(size, dim, coeffs=None, offset=None):
    """An acceleration that differs at every node and in every component, with no symmetry under a swap of axes:
    a[d] = offset[d] + sum_k coeffs[d][k] * x_k over the real nodes, float64 [dim, (nz,) ny, nx]; coefficients of order
    1e-5 / extent with distinct, non-commensurate ratios."""
    shape = tuple(reversed(size))
    idx = np.indices(shape).astype(np.float64)[::-1]          # x, y[, z]
    if coeffs is None:
        base = np.array([[1.0, np.sqrt(2.0), np.sqrt(3.0)], [-np.sqrt(5.0), np.sqrt(7.0) / 2, 1.0 / np.sqrt(11.0)],
                         [np.sqrt(13.0) / 3, -1.0 / np.sqrt(17.0), np.sqrt(19.0) / 4]])
        coeffs = 1e-5 * base[:dim, :dim] / np.array(size, dtype=np.float64)[None, :]
    if offset is None:
        offset = 1e-5 * np.array([0.3, -0.7, 0.45])[:dim]
    return np.stack([offset[d] + sum(coeffs[d][k] * idx[k] for k in range(dim)) for d in range(dim)])
