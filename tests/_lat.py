"""Shared set-up of the D3Q15 / D3Q27 tests: simulation classes for the runner's side (GPU) and for the numpy twin
(tests/_lat_twin.py), both built from the same host layer and started from the same global fields."""
import numpy as np

from sailfish_amd import sym
from sailfish_amd.geo import LBGeometry3D
from sailfish_amd.lb_base import LBForcedSim
from sailfish_amd.lb_single import LBFluidSim
from sailfish_amd.node_type import NTFullBBWall, NTHalfBBWall
from sailfish_amd.subdomain import Subdomain3D, SubdomainSpec3D

LATTICES = ['D3Q15', 'D3Q27']
DTYPE = {'single': np.float32, 'double': np.float64}
ACCEL = (3e-5, -2e-5, 1e-5)          # three distinct components, so that no axis mix-up can hide

# the boxes of the issue: size (x, y, z), walls, force scheme
WALL_BOX = dict(size=(20, 12, 10), walls='full', force='guo')          # full-way walls on all faces, Guo force
CHANNEL = dict(size=(18, 6, 10), walls='half', force='edm')            # between half-way walls (z faces), EDM
PERIODIC_BOX = dict(size=(20, 12, 10), walls=None, force='guo')        # the wall box's periodic sibling


def global_fields(gshape, seed=5, amplitude=0.03):
    """rho and v on the global grid (numpy axis order z, y, x): a few random Fourier modes each -- smooth, periodic, rho in
    1 +- amplitude, |v_d| <= amplitude.  Defined globally, so every decomposition starts from the same state."""
    rng = np.random.RandomState(seed)
    z, y, x = np.meshgrid(*[np.arange(n) / float(n) for n in gshape], indexing='ij')
    out = []
    for _ in range(4):
        a = np.zeros(gshape)
        for _ in range(3):
            k = rng.randint(1, 3, size=3)
            ph = rng.uniform(0, 2 * np.pi, size=3)
            a += np.sin(2 * np.pi * k[0] * z + ph[0]) * np.sin(2 * np.pi * k[1] * y + ph[1]) * np.sin(2 * np.pi * k[2] * x + ph[2])
        out.append(amplitude * a / 3.0)
    return 1.0 + out[0], out[1:]


def make_sim(walls=None, accel=None, uniform=False, seed=5):
    """walls: None | 'full' (NTFullBBWall on all six faces) | 'half' (NTHalfBBWall on both z faces); accel: body force."""

    class Box(Subdomain3D):
        def boundary_conditions(self, hx, hy, hz):
            if walls == 'full':
                m = (hx == 0) | (hx == self.gx - 1) | (hy == 0) | (hy == self.gy - 1) | (hz == 0) | (hz == self.gz - 1)
                self.set_node(m, NTFullBBWall)
            elif walls == 'half':
                self.set_node((hz == 0) | (hz == self.gz - 1), NTHalfBBWall)

        def initial_conditions(self, sim, hx, hy, hz):
            if uniform:
                sim.rho[:] = 1.0
                return
            rho, v = global_fields((self.gz, self.gy, self.gx), seed)
            where = (hz, hy, hx)
            sim.rho[:] = rho[where]
            for c, a in zip((sim.vx, sim.vy, sim.vz), v):
                c[:] = a[where]

    class Sim(LBFluidSim, LBForcedSim):
        subdomain = Box

        def __init__(self, config):
            super(Sim, self).__init__(config)
            if accel is not None:
                self.add_body_force(tuple(accel))

    return Sim


def block_geometry(cuts):
    """Geometry class cutting the domain into a block grid: cuts = per-axis lists of cut positions (x first)."""
    class Geo(LBGeometry3D):
        def subdomains(self, n=None):
            edges = [[0] + list(c) + [g] for c, g in zip(cuts, self.gsize)]
            out = []
            for k in range(len(edges[2]) - 1):
                for j in range(len(edges[1]) - 1):
                    for i in range(len(edges[0]) - 1):
                        lo = (edges[0][i], edges[1][j], edges[2][k])
                        hi = (edges[0][i + 1], edges[1][j + 1], edges[2][k + 1])
                        out.append(SubdomainSpec3D(lo, tuple(b - a for a, b in zip(lo, hi))))
            return out
    return Geo


def config(grid, size, walls=None, force=None, pattern='AB', precision='double', fused=True, visc=0.05, **over):
    per = dict(periodic_x=walls != 'full', periodic_y=walls != 'full', periodic_z=walls is None)
    cfg = dict(lat_nx=size[0], lat_ny=size[1], lat_nz=size[2], grid=grid, access_pattern=pattern, precision=precision,
               hip_fused_periodic=fused, visc=visc, force_implementation=force or 'guo', **per)
    cfg.update(over)
    return cfg


def case(grid, box, **over):
    """(simulation class, config) of one of the boxes above."""
    kw = dict(box)
    kw.update(over)
    size, walls, force = kw.pop('size'), kw.pop('walls'), kw.pop('force')
    accel = kw.pop('accel', ACCEL if force else None)
    return make_sim(walls, accel), config(grid, size, walls, force, **kw)


def wet_mask(size, walls):
    wet = np.ones(tuple(reversed(size)), dtype=bool)
    if walls == 'full':
        wet[0] = wet[-1] = False
        wet[:, 0] = wet[:, -1] = False
        wet[:, :, 0] = wet[:, :, -1] = False
    return wet


def merged(ctrl, what):
    """A field ('rho', 'v0' ..) or the populations ('dist') of every runner of a controller on the global grid."""
    r0 = ctrl.runners[0]
    gshape = tuple(reversed(r0._global_size))
    out = np.zeros(((r0._sim.grid.Q,) if what == 'dist' else ()) + gshape, dtype=r0.float)
    for r in ctrl.runners:
        sp = r._spec
        sl = tuple(slice(o, o + n) for o, n in zip(reversed(sp.location), reversed(sp.size)))
        if what == 'dist':
            d = r._debug_get_dist()
            out[(slice(None),) + sl] = d[(slice(None),) + tuple(sp._nonghost_slice)]
        elif what[0] == 'v':
            out[sl] = r._sim.v[int(what[1:])]
        else:
            out[sl] = getattr(r._sim, what)
    return out


def run_gpu(sim_cls, cfg, steps, geo=LBGeometry3D):
    from sailfish_amd.controller import LBSimulationController
    cfg = dict(cfg, max_iters=steps, quiet=True, perf_stats_every=0)
    ctrl = LBSimulationController(sim_cls, geo, default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    return ctrl
