"""Set-ups shared by the tests of the shallow-water model (tests/test_sw_twin.py, tests/test_gpu_sw.py): box descriptors
with the equilibrium switch, channels with full-way, half-way or slip walls on the two y faces, humps and seeded states.
The node-type table holds the kinds a shallow-water module serves and no other (one value-carrying kind in the table is
enough for a refusal).  Test-only."""
import numpy as np

from sailfish_amd import hipabi, sym
from sailfish_amd.box import make_box_desc
from tests import _geometry as geo

GRID = sym.D2Q9
TYPE_KIND = [hipabi.SLF_NK_FLUID, hipabi.SLF_NK_GHOST, hipabi.SLF_NK_FULL_BB, hipabi.SLF_NK_SLIP, hipabi.SLF_NK_HALF_BB]
T_FLUID, T_GHOST, T_FULLBB, T_SLIP, T_HALFBB = range(5)
assert (T_FLUID, T_GHOST, T_FULLBB, T_HALFBB) == (geo.T_FLUID, geo.T_GHOST, geo.T_FULLBB, geo.T_HALFBB)
DTYPE = {'single': np.float32, 'double': np.float64}


def g32(g):
    """The gravity as a module has it: slf_module_desc::gravity is a float, whatever the module's precision."""
    return float(np.float32(g))


def walled_map(desc, kind):
    """Walls on the rows y = 1 and y = max, x periodic: 'full' / 'half' (link tags, which see the periodic neighbours) /
    'slip' (inward normal +y below: orientation 2, -y above: orientation 4)."""
    m = geo.empty_map(desc)
    ny, nx = desc.lat_ny - 2, desc.lat_nx - 2
    if kind == 'slip':
        m[0, 1, 1:nx + 1] = geo.encode(T_SLIP, orientation=2)
        m[0, ny, 1:nx + 1] = geo.encode(T_SLIP, orientation=4)
        return m
    t = T_FULLBB if kind == 'full' else T_HALFBB
    m[0, 1, 1:nx + 1] = geo.encode(t)
    m[0, ny, 1:nx + 1] = geo.encode(t)
    if kind == 'full':
        return m
    mm = m.copy()
    mm[:, :, 0] = mm[:, :, nx]
    mm[:, :, nx + 1] = mm[:, :, 1]
    for y in (1, ny):
        for x in range(1, nx + 1):
            m[0, y, x] = geo.encode(T_HALFBB, orientation=geo.link_tags(GRID, mm, 0, y, x, wet_types=(T_FLUID, T_HALFBB)))
    return m


def box_desc(size, pattern, precision, gravity=0.05, visc=0.01, walls=None, fused=1, accel=None, accel_field=False,
             force='guo'):
    """(descriptor, periodic axes, node-map builder or None).  walls: None (fully periodic), 'full', 'half', 'slip'."""
    periodic = (True, walls is None, False)
    kw = {}
    if walls is not None:
        kw = dict(fluid_only=False, type_kind=TYPE_KIND, nt_bits=geo.NT_BITS, use_link_tags=True)
    desc = make_box_desc(GRID, size, precision=precision, access_pattern=pattern, visc=visc,
                         periodic_fused=[int(fused and p) for p in periodic], accel=accel, accel_field=accel_field, **kw)
    desc.force_implementation = hipabi.SLF_FORCE_EDM if force == 'edm' else hipabi.SLF_FORCE_GUO
    desc.equilibrium = hipabi.SLF_EQ_SHALLOW_WATER
    desc.gravity = gravity
    return desc, periodic, (None if walls is None else (lambda d: walled_map(d, walls)))


def hump(size, amplitude=0.4, width=None):
    """The Gaussian hump of examples/fs_gaussian.py on nx x ny real nodes: depth [ny, nx], the fluid at rest."""
    nx, ny = size
    width = min(nx, ny) / 12.0 if width is None else width
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    h = 1.0 + amplitude * np.exp(-((x - nx / 2.0) ** 2 + (y - ny / 2.0) ** 2) / width ** 2)
    return h, [np.zeros_like(h), np.zeros_like(h)]


def seeded(size, seed=77):
    """h = 1 + 0.1 U, |v| < 0.03, different at every node and in every component."""
    rng = np.random.RandomState(seed)
    shape = (size[1], size[0])
    return 1.0 + 0.1 * rng.rand(*shape), [0.03 * (2.0 * rng.rand(*shape) - 1.0) for _ in range(2)]


def start(sim, fields):
    sim.set_fields(*fields)
    sim.initial_conditions()
    return sim


# ---- through the controller (the host tests on the CPU backend, the GPU tests on the HIP backend) --------------------------

def global_fields(gshape, kind='seeded', seed=77):
    """h and v on the global grid [ny, nx]: defined globally, so every decomposition starts from the same state."""
    ny, nx = gshape
    if kind == 'hump':
        return hump((nx, ny))
    if kind == 'cosine':
        x = np.arange(nx, dtype=np.float64)
        h = np.tile(1.0 + 0.01 * np.cos(2.0 * np.pi * x / nx), (ny, 1))
        return h, [np.zeros_like(h), np.zeros_like(h)]
    return seeded((nx, ny), seed)


def make_sim(walls=None, forces=(), fields='seeded', base=None):
    """An LBFreeSurface simulation with LBForcedSim.  walls: None | 'full' | 'half' | 'slip' on the two y faces, or a node
    type class for them; forces: what add_body_force takes, one call each."""
    from sailfish_amd import node_type as nt
    from sailfish_amd.lb_base import LBForcedSim
    from sailfish_amd.lb_single import LBFreeSurface
    from sailfish_amd.subdomain import Subdomain2D

    class Box(Subdomain2D):
        def boundary_conditions(self, hx, hy):
            if walls == 'full':
                self.set_node((hy == 0) | (hy == self.gy - 1), nt.NTFullBBWall)
            elif walls == 'half':
                self.set_node((hy == 0) | (hy == self.gy - 1), nt.NTHalfBBWall)
            elif walls == 'slip':
                self.set_node(hy == 0, nt.NTSlip(orientation=GRID.vec_to_dir([0, 1])))
                self.set_node(hy == self.gy - 1, nt.NTSlip(orientation=GRID.vec_to_dir([0, -1])))
            elif walls is not None:
                self.set_node(hy == 0, walls)

        def initial_conditions(self, sim, hx, hy):
            h, v = global_fields((self.gy, self.gx), fields)
            sim.rho[:] = h[hy, hx]
            sim.vx[:] = v[0][hy, hx]
            sim.vy[:] = v[1][hy, hx]

    class Sim(base or LBFreeSurface, LBForcedSim):
        subdomain = Box

        def __init__(self, config):
            super(Sim, self).__init__(config)
            for f in forces:
                self.add_body_force(f)

    return Sim


def config(size, walls=None, pattern='AB', precision='double', fused=True, gravity=0.05, visc=0.01, **over):
    cfg = dict(lat_nx=size[0], lat_ny=size[1], access_pattern=pattern, precision=precision, hip_fused_periodic=fused,
               gravity=gravity, visc=visc, periodic_x=True, periodic_y=walls is None)
    cfg.update(over)
    return cfg


def strip_geometry(axis, cut):
    """Two subdomains, cut at `cut` along axis 0 (x) or 1 (y)."""
    from sailfish_amd.geo import LBGeometry2D
    from sailfish_amd.subdomain import SubdomainSpec2D

    class Geo(LBGeometry2D):
        def subdomains(self, n=None):
            gx, gy = self.gsize
            if axis == 0:
                return [SubdomainSpec2D((0, 0), (cut, gy)), SubdomainSpec2D((cut, 0), (gx - cut, gy))]
            return [SubdomainSpec2D((0, 0), (gx, cut)), SubdomainSpec2D((0, cut), (gx, gy - cut))]
    return Geo


def run(sim_cls, cfg, steps, geo=None, **over):
    from sailfish_amd.controller import LBSimulationController
    from sailfish_amd.geo import LBGeometry2D
    cfg = dict(cfg, max_iters=steps, quiet=True, perf_stats_every=0, output='', **over)
    ctrl = LBSimulationController(sim_cls, geo or LBGeometry2D, default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    return ctrl
