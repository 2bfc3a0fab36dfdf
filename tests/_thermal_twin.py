"""numpy twin of the temperature lattice of a thermal flow (device code: csrc/slf_thermal.hip behind the C ABI's
slf_thermal_* entry points), restated from the model's rules independently of the kernel file -- arrays over the wet nodes,
one numpy operation per floating-point operation, in the module's format R:

    directions 0 rest, 1 +x, 2 -x, 3 +y, 4 -y, 5 +z, 6 -z;  D2Q5: w0 = 1/3, w = 1/6, k = 3;  D3Q7: w0 = 1/4, w = 1/8, k = 4
    omega_T = R(1 / tau_T), kappa = (tau_T - 1/2) / k
    pull     n = x - e_i, wrapped on the periodic axes
             n real and wet:      g_i = src[i][n]
             n real and not wet:  Tw = wall_temperature[n];  finite: g_i = (2 w_i) * Tw - src[opp i][x];  else g_i = src[opp i][x]
             n not a real node:   g_i = src[opp i][x]
    T        = ((g0 + g1) + g2) + ...
    fixed    (modules with a node map) wall_temperature[x] finite at the wet node: T = Tw, g_i = geq_i
    collide  eu_i = +-u[d];  geq_i = (w_i * T) * (1 + k * eu_i);  dst[i][x] = g_i + omega_T * (geq_i - g_i)
    store    T[x] = T;  field[d][x] = b[d] * (T - T_ref)

A step reads copy it & 1 and writes the other; nodes that are not wet are never written.  ThermalTwin is the lattice alone,
on a velocity handed to it; ThermalTwinBox composes it with tests/_accf_twin.AccfTwinBox for the fluid step (BGK), the thermal
step behind the sweep: the sweep of step n is forced with the T of step n - 1, the temperature collides with the u of step n.
Test-only."""
import numpy as np

from sailfish_amd import hipabi
from tests import _lat_twin as lt
from tests._accf_twin import AccfTwinBox


def lattice(dim):
    """(Q, weights, k) of D2Q5 / D3Q7 as Python floats."""
    if dim == 2:
        return 5, [1.0 / 3.0] + [1.0 / 6.0] * 4, 3.0
    return 7, [0.25] + [0.125] * 6, 4.0


def tau_of(kappa, dim):
    return 0.5 + lattice(dim)[2] * kappa


class ThermalTwin(object):
    def __init__(self, dim, dtype, lat, shape, periodic, wet, has_map, tau_t, t_ref, b, field, fill=np.nan):
        """lat / shape: (nz, ny, nx) with the ghost layer / of the padded arrays (nz = 1 in 2-D); periodic: per axis x, y, z;
        wet: bool over `shape` or None (every real node is wet); field: [dim] + shape, the acceleration field the step
        writes.  The populations start as `fill` everywhere."""
        self.dim, self.R = dim, dtype
        self.Q, w, k = lattice(dim)
        R = dtype
        self.w = [R(x) for x in w]
        self.w2 = [R(2.0) * R(x) for x in w]
        self.k = R(k)
        self.omega = R(1.0 / tau_t)
        self.t_ref = R(t_ref)
        self.b = [R(x) for x in b]
        self.lat, self.shape = tuple(lat), tuple(shape)
        self.periodic = [bool(p) for p in periodic] + [False] * (3 - len(periodic))
        self.has_map = bool(has_map)
        self.wet = np.ones(self.shape, dtype=bool) if wet is None else np.asarray(wet, dtype=bool)
        self.g = [np.full((self.Q,) + self.shape, fill, dtype=R) for _ in (0, 1)]
        self.T = np.full(self.shape, fill, dtype=R)
        self.wall_t = np.full(self.shape, np.nan, dtype=R)
        self.field = field
        self.it = 0
        zr = np.arange(1, lat[0] - 1) if dim == 3 else np.arange(1)
        z, y, x = [a.ravel() for a in np.meshgrid(zr, np.arange(1, lat[1] - 1), np.arange(1, lat[2] - 1), indexing='ij')]
        keep = self.wet[z, y, x]
        self.here = (z[keep], y[keep], x[keep])            # the wet real nodes

    @staticmethod
    def opp(i):
        return 0 if i == 0 else (i + 1 if i & 1 else i - 1)

    def real_view(self, arr):
        if self.dim == 3:
            return arr[..., 1:self.lat[0] - 1, 1:self.lat[1] - 1, 1:self.lat[2] - 1]
        return arr[..., 0, 1:self.lat[1] - 1, 1:self.lat[2] - 1]

    def geq(self, i, T, u):
        R = self.R
        if i == 0:
            eu = np.zeros_like(T)
        else:
            d = (i - 1) // 2
            eu = u[d] if i & 1 else -u[d]
        return (self.w[i] * T) * (R(1) + self.k * eu)

    def _store(self, T):
        self.T[self.here] = T
        dt = T - self.t_ref
        for d in range(self.dim):
            self.field[d][self.here] = self.b[d] * dt

    def init(self, v):
        """g[0] = geq(T, v) and the buoyancy of T, at the wet nodes.  v: dim arrays over `shape`."""
        T = self.T[self.here]
        u = [c[self.here] for c in v[:self.dim]]
        with np.errstate(all='ignore'):
            for i in range(self.Q):
                self.g[0][(i,) + self.here] = self.geq(i, T, u)
            self._store(T)
        self.it = 0

    def step(self, v):
        src, dst = self.g[self.it & 1], self.g[1 - (self.it & 1)]
        here = self.here
        gp = [src[(0,) + here]]
        with np.errstate(all='ignore'):
            for i in range(1, self.Q):
                d = (i - 1) // 2
                ax = 2 - d                                   # arrays are z, y, x
                sign = 1 if i & 1 else -1
                cn = here[ax] - sign
                n = self.lat[ax]
                low, high = cn < 1, cn > n - 2
                real = ~(low | high) | self.periodic[d]
                cn = np.where(low, n - 2, np.where(high, 1, cn))
                at = tuple(cn if a == ax else here[a] for a in range(3))
                own = src[(self.opp(i),) + here]
                tw = self.wall_t[at]
                walled = np.where(np.isfinite(tw), self.w2[i] * tw - own, own)
                gp.append(np.where(real, np.where(self.wet[at], src[(i,) + at], walled), own))
            T = gp[0]
            for i in range(1, self.Q):
                T = T + gp[i]
            u = [c[here] for c in v[:self.dim]]
            if self.has_map:
                tw = self.wall_t[here]
                fixed = np.isfinite(tw)
                T = np.where(fixed, tw, T)
                gp = [np.where(fixed, self.geq(i, T, u), gp[i]) for i in range(self.Q)]
            for i in range(self.Q):
                dst[(i,) + here] = gp[i] + self.omega * (self.geq(i, T, u) - gp[i])
            self._store(T)
        self.it += 1

    def current(self):
        return self.g[self.it & 1]


class ThermalTwinBox(AccfTwinBox):
    """The step sequence of sailfish_amd.box.BoxSim with sailfish_amd.thermal.ThermalLattice behind every sweep, on the
    twins.  temperature, wall_temperature: over the real nodes ((nz,) ny, nx); wall_temperature None: NaN everywhere."""

    def __init__(self, desc, periodic, node_map, temperature, wall_temperature, tau_t, t_ref, b, fill=np.nan):
        dim = 2 if desc.lattice == hipabi.SLF_D2Q9 else 3
        shape = tuple(reversed([desc.lat_nx - 2, desc.lat_ny - 2] + ([desc.lat_nz - 2] if dim == 3 else [])))
        super(ThermalTwinBox, self).__init__(desc, periodic, node_map, accel_field=np.zeros((dim,) + shape), fill=fill)
        d = desc
        wet = None
        if not d.fluid_only and self.node_map is not None:
            kind = np.array(list(d.type_kind[:d.n_types]))[self.node_map & np.uint32(d.nt_type_mask)]
            wet = np.isin(kind, lt.WET)
        self.t = ThermalTwin(dim, self.dtype, (d.lat_nz, d.lat_ny, d.lat_nx), self.shape, periodic, wet, wet is not None,
                             tau_t, t_ref, b, self.accel_field, fill)
        self.real_view(self.t.T)[...] = np.asarray(temperature, dtype=np.float64)
        if wall_temperature is not None:
            self.real_view(self.t.wall_t)[...] = np.asarray(wall_temperature, dtype=np.float64)

    def initial_conditions(self):
        super(ThermalTwinBox, self).initial_conditions()
        self.t.init(self.v)

    def lattice_step(self):
        """The thermal step alone, with the velocity as it stands."""
        self.t.step(self.v)

    def step(self, save_macro=True, region=None):
        assert save_macro and region is None         # the temperature collides with the v of every step
        super(ThermalTwinBox, self).step(save_macro=True)
        self.t.step(self.v)

    def temperature(self):
        return np.array(self.real_view(self.t.T))

    def velocity(self):
        return [np.array(self.real_view(c)) for c in self.v[:self.dim]]
