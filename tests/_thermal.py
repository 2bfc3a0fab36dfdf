"""Set-ups shared by the tests of the thermal flows (tests/test_thermal_twin.py, tests/test_thermal_host.py,
tests/test_gpu_thermal.py): the geometries of the parity tests, the device-side box with a temperature lattice, and the
physics cases -- written once against the interface the twin (tests/_thermal_twin.ThermalTwinBox) and the device box
(BoxWithThermal) share: set_fields, initial_conditions, step, lattice_step, temperature, velocity.  Test-only."""
import numpy as np

from sailfish_amd import sym
from sailfish_amd.box import make_box_desc
from sailfish_amd import hipabi
from tests import _accf
from tests import _geometry as geo
from tests._thermal_twin import tau_of

GRIDS = {2: sym.D2Q9, 3: sym.D3Q19}
POISON = 1e30          # wall_temperature of ghost and padding entries: finite, so a launch that read one would show


# ---- geometries ----------------------------------------------------------------------------------------------------------------
# kind -> periodic axes (x, y, z) and what the node map holds.  Sizes are (nx, ny[, nz]) real nodes.
#   'periodic'  no map, every axis periodic
#   'open_x'    no map, x periodic only: the other faces are open (the pull from beyond them takes the node's own opposite
#               population; the flow keeps what SetInitialConditions left in the slots nothing streams into)
#   'open'      no map, no axis periodic
#   'block'     map, every axis periodic: an interior solid block (finite wall temperature on its lower half, NaN above) and
#               a wet node with a fixed temperature
#   'channel'   map, x periodic only (x and z in 3-D): low y face full-way walls (finite wall temperature on the first half
#               of x, NaN on the second), high y face a half-way wall with the unused layer behind it carrying a
#               temperature; the block and the fixed node.  No half-way wall node has a full-way wall node for a neighbour:
#               both would supply the same population of the flow, in an order the sweep does not define
#   'box'       map, no axis periodic: full-way walls on every face (finite on the low x face), the block and the fixed node
KINDS = {'periodic': (True, True, True), 'open_x': (True, False, False), 'open': (False, False, False), 'block': (True, True, True), 'channel': (True, False, True),
         'box': (False, False, False)}

NO_MAP = ('periodic', 'open_x', 'open')


def geometry(kind, size, pattern, precision, model='bgk', visc=0.05, fused=1):
    """(descriptor, periodic, node map or None, wall_temperature over the real nodes)."""
    dim = len(size)
    grid = GRIDS[dim]
    periodic = tuple(KINDS[kind][:dim]) + (False,) * (3 - dim)
    kw = {}
    if kind not in NO_MAP:
        kw = dict(fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, use_link_tags=True)
    desc = make_box_desc(grid, size, model=model, precision=precision, access_pattern=pattern, visc=visc,
                         periodic_fused=[int(fused and p) for p in periodic], accel_field=True, **kw)
    desc.force_implementation = hipabi.SLF_FORCE_GUO
    shape = tuple(reversed(size))
    wall_t = np.full(shape, np.nan)
    if kind in NO_MAP:
        return desc, periodic, None, wall_t
    types = np.full((1,) + shape if dim == 2 else shape, geo.T_FLUID, dtype=np.int64)       # (nz, ny, nx) real nodes
    wt = wall_t.reshape(types.shape)
    nz, ny, nx = types.shape
    if kind == 'channel':
        types[:, 0, :] = geo.T_FULLBB
        wt[:, 0, :nx // 2] = 1.0
        types[:, ny - 1, :] = geo.T_UNUSED
        wt[:, ny - 1, :] = 0.25
        types[:, ny - 2, :] = geo.T_HALFBB
    elif kind == 'box':
        types[:, 0, :] = types[:, ny - 1, :] = geo.T_FULLBB
        types[:, :, 0] = types[:, :, nx - 1] = geo.T_FULLBB
        wt[:, :, 0] = 0.75
        if dim == 3:
            types[0] = types[nz - 1] = geo.T_FULLBB
    zc = nz // 2
    y0, rows = 2, (2 if ny >= 8 else 1)                        # (one row in the low boxes: a fluid row on either side)
    types[zc, y0:y0 + rows, 20:23] = geo.T_FULLBB              # the block
    wt[zc, y0, 20:23] = 0.5
    fixed = (zc, y0, 40)                                        # a wet node held at a temperature
    assert types[fixed] == geo.T_FLUID
    wt[fixed] = 0.625
    # codes; half-way walls get their link tags from the map with the periodic images in its ghost layer
    pad = [(1, 1) if dim == 3 else (0, 0), (1, 1), (1, 1)]
    padded = np.pad(types, pad, mode='constant', constant_values=geo.T_GHOST)
    for ax, d in ((2, 0), (1, 1), (0, 2)):
        if d < dim and periodic[d]:
            sl = [slice(None)] * 3
            lo, hi, first, last = list(sl), list(sl), list(sl), list(sl)
            lo[ax], hi[ax], first[ax], last[ax] = 0, -1, 1, -2
            padded[tuple(lo)] = padded[tuple(last)]
            padded[tuple(hi)] = padded[tuple(first)]
    m = geo.empty_map(desc)
    zoff = 1 if dim == 3 else 0
    for z, y, x in np.argwhere(types != geo.T_FLUID):
        t = int(types[z, y, x])
        tag = geo.link_tags(grid, padded, z + zoff, y + 1, x + 1) if t == geo.T_HALFBB else 0
        m[z + zoff, y + 1, x + 1] = geo.encode(t, orientation=tag)
    return desc, periodic, m, wall_t


def start(sim, kind, size):
    """Seeded rho and v (tests/_accf.start_fields), then the initial conditions of flow and temperature.  The map-free boxes
    with open faces get a resting reservoir first -- rho = 1, v = 0 in the ghost entries of the fields, where the others hold
    the +inf sentinel: the in-place sweep pulls out of the ghost slots what SetInitialConditions left there, and the flow
    next to an open face would otherwise not be finite (on the device and in the twin alike)."""
    box = getattr(sim, 'box', sim)
    if kind in ('open_x', 'open'):
        box.rho[...] = 1.0
        for c in box.v:
            c[...] = 0.0
    return _accf.start(sim, size, len(size))


def start_temperature(size, seed=5):
    """0.3 .. 0.7, different at every node."""
    return 0.3 + 0.4 * np.random.RandomState(seed).rand(*tuple(reversed(size)))


# ---- the device side -------------------------------------------------------------------------------------------------------------

class BoxWithThermal(object):
    """sailfish_amd.box.BoxSim with sailfish_amd.thermal.ThermalLattice behind its step: the step sequence of
    tests/_thermal_twin.ThermalTwinBox on the device.  Ghost and padding entries hold NaN (T, the populations, the field)
    or a finite poison (wall_temperature)."""

    def __init__(self, backend, desc, periodic, node_map, temperature, wall_temperature, tau_t, t_ref, b, fill=np.nan):
        from sailfish_amd import thermal
        from sailfish_amd.box import BoxSim
        dim = 2 if desc.lattice == hipabi.SLF_D2Q9 else 3
        shape = tuple(reversed([desc.lat_nx - 2, desc.lat_ny - 2] + ([desc.lat_nz - 2] if dim == 3 else [])))
        self.box = box = BoxSim(backend, desc, periodic=periodic, node_map=node_map, accel_field=np.zeros((dim,) + shape),
                                accel_field_fill=fill)
        self.backend, self.dim = backend, dim
        self.T = np.full(box.shape, fill, dtype=box.dtype)
        box.real_view(self.T)[...] = temperature
        self.wall_t = np.full(box.shape, POISON, dtype=box.dtype)
        box.real_view(self.wall_t)[...] = np.nan if wall_temperature is None else wall_temperature
        off = backend.dist_align_offset(box.dtype().itemsize)
        self.gpu_T = backend.alloc_buf(like=self.T, align_offset=off)
        self.gpu_wall_t = backend.alloc_buf(like=self.wall_t, align_offset=off)
        kappa = (tau_t - 0.5) / (3.0 if dim == 2 else 4.0)
        self.lat = thermal.ThermalLattice(backend, box.module, box.dtype, dim, box.shape, periodic[:dim], kappa, t_ref, b, fill=fill)
        assert abs(self.lat.tau - tau_t) < 1e-15
        self.it = 0

    def set_fields(self, rho, v):
        self.box.set_fields(rho, v)

    def initial_conditions(self):
        self.box.initial_conditions()
        self.lat.init(self.box.gpu_map, self.gpu_T, self.box.gpu_v, self.box.stream)
        self.it = 0

    def lattice_step(self):
        """The thermal launch alone, with the velocity as it stands."""
        self.lat.back(self.it, self.box.gpu_map, self.box.gpu_v, self.gpu_wall_t, self.gpu_T, self.box.stream)
        self.it += 1

    def step(self):
        self.box.step(save_macro=True)
        self.lattice_step()

    def populations(self, copy):
        return self.lat.populations(copy, self.box.stream)

    def temperature_array(self):
        self.box.sync()
        self.backend.from_buf(self.gpu_T)
        return np.array(self.T)

    def wall_temperature_array(self):
        self.box.sync()
        self.backend.from_buf(self.gpu_wall_t)
        return np.array(self.wall_t)

    def field(self):
        self.box.sync()
        self.backend.from_buf(self.box.gpu_accel_field)
        return np.array(self.box.accel_field)

    def temperature(self):
        return np.array(self.box.real_view(self.temperature_array()))

    def velocity(self):
        _, v = self.box.fetch_fields()
        return [np.array(self.box.real_view(c)) for c in v[:self.dim]]

    def release(self):
        self.box.sync()
        self.lat.release()
        self.backend.free_buf(self.gpu_T)
        self.backend.free_buf(self.gpu_wall_t)
        self.box.release()


def twin_box(desc, periodic, node_map, temperature, wall_temperature, tau_t, t_ref, b):
    from tests._thermal_twin import ThermalTwinBox
    return ThermalTwinBox(desc, periodic, node_map, temperature, wall_temperature, tau_t, t_ref, b)


# ---- physics cases.  make(desc, periodic, node_map, T0, wall_t, tau_t, t_ref, b) builds the twin or the
# device box; every function returns plain numbers. ------------------------------------------------------------------------------

# (b) pure conduction between plates: (tau_T, H, steps); the steps are a few dozen e-folding times H^2 / (pi^2 kappa)
CONDUCTION = [(1.0, 16, 6000), (0.6, 8, 8000), (1.7, 8, 2000)]


def conduction(make, precision, tau_t, H, steps):
    """Largest deviation of the steady profile from the straight line through the link mid-points, in units of eps."""
    size = (4, H + 2)
    desc, periodic, map_fn = _accf.box_desc(sym.D2Q9, size, 'AB', precision, 'guo', 'full', 1, accel_field=True)
    shape = tuple(reversed(size))
    wall_t = np.full(shape, np.nan)
    wall_t[0], wall_t[-1] = 1.0, 0.0
    sim = make(desc, periodic, map_fn(desc), np.full(shape, 0.5), wall_t, tau_t, 0.0, [0.0, 0.0])
    sim.set_fields(np.ones(shape), [np.zeros(shape)] * 2)
    sim.initial_conditions()
    for _ in range(steps):
        sim.lattice_step()
    want = 1.0 - (np.arange(1, H + 1) - 0.5) / H
    got = sim.temperature()[1:-1].astype(np.float64)
    eps = np.finfo(np.float32 if precision == 'single' else np.float64).eps
    return float(np.abs(got - want[:, None]).max() / eps)


# (c) a sine wave advected by a uniform velocity
WAVE = dict(size=(70, 8), u=0.05, kappa=0.1, amplitude=0.1, mean=0.5, steps=400)


def advected_wave(make, precision):
    """(relative L2 error of the temperature perturbation against amplitude exp(-kappa k^2 t) sin(k (x - u t)), relative
    error of the fitted decay rate, relative error of the fitted phase speed) after WAVE['steps'] steps."""
    w = WAVE
    nx, ny = w['size']
    desc, periodic, _ = _accf.box_desc(sym.D2Q9, w['size'], 'AB', precision, 'guo', None, 1, accel_field=True)
    x = np.arange(nx)
    k = 2.0 * np.pi / nx
    T0 = np.tile(w['mean'] + w['amplitude'] * np.sin(k * x), (ny, 1))
    sim = make(desc, periodic, None, T0, None, tau_of(w['kappa'], 2), 0.0, [0.0, 0.0])
    sim.set_fields(np.ones((ny, nx)), [np.full((ny, nx), w['u']), np.zeros((ny, nx))])
    sim.initial_conditions()
    n = w['steps']
    for _ in range(n):
        sim.lattice_step()
    got = sim.temperature().astype(np.float64)
    exact = w['amplitude'] * np.exp(-w['kappa'] * k * k * n) * np.sin(k * (x - w['u'] * n))
    l2 = float(np.sqrt(((got - w['mean'] - exact[None, :]) ** 2).sum() / (np.tile(exact, (ny, 1)) ** 2).sum()))
    mode = lambda T: (T.mean(axis=0) * np.exp(-1j * k * x)).sum() * 2.0 / nx          # noqa: E731
    c0, c1 = mode(T0), mode(got)
    rate = -np.log(abs(c1) / abs(c0)) / n
    speed = -np.angle(c1 / c0) / (k * n)
    return l2, float(rate / (w['kappa'] * k * k) - 1.0), float(speed / w['u'] - 1.0)


# (d) Rayleigh-Benard onset between full-way walls: Pr = 1, critical Rayleigh number 1707.76
RB = dict(size=(32, 18), nu=0.03, steps=2000, seed=1e-3, above=5000.0, below=800.0)


def rayleigh_benard(make, precision, Ra):
    """(kinetic energy at the end / at mid-run, peak speed): the fluid nodes of a box heated from below, T = 1 at the lower
    and 0 at the upper wall mid-points, T_ref = 1/2, started from the conduction profile plus one seeded roll pair."""
    nx, ny = RB['size']
    H = ny - 2
    nu = kappa = RB['nu']
    b = Ra * nu * kappa / float(H ** 3)
    desc, periodic, map_fn = _accf.box_desc(sym.D2Q9, RB['size'], 'AB', precision, 'guo', 'full', 1, accel_field=True, visc=nu)
    y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    T0 = 1.0 - (y - 0.5) / H + RB['seed'] * np.sin(2.0 * np.pi * x / nx) * np.sin(np.pi * (y - 0.5) / H)
    wall_t = np.full((ny, nx), np.nan)
    wall_t[0], wall_t[-1] = 1.0, 0.0
    sim = make(desc, periodic, map_fn(desc), T0, wall_t, tau_of(kappa, 2), 0.5, [0.0, b])
    sim.set_fields(np.ones((ny, nx)), [np.zeros((ny, nx))] * 2)
    sim.initial_conditions()

    def energy():
        vx, vy = [c[1:-1].astype(np.float64) for c in sim.velocity()]
        return float(0.5 * (vx ** 2 + vy ** 2).sum()), float(np.sqrt(vx ** 2 + vy ** 2).max())

    for _ in range(RB['steps'] // 2):
        sim.step()
    mid, peak_mid = energy()
    for _ in range(RB['steps'] - RB['steps'] // 2):
        sim.step()
    end, peak_end = energy()
    return end / mid, max(peak_mid, peak_end)
