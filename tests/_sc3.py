"""Shared set-up of the ternary Shan-Chen tests: the simulation class on the runner's side and the numpy twin
(tests/_scn_twin.py) of the same box, started from the same global fields."""
import numpy as np

from sailfish_amd import sym
from sailfish_amd.geo import LBGeometry2D, LBGeometry3D
from sailfish_amd.lb_ternary import LBTernaryFluidShanChen
from sailfish_amd.node_type import NTFullBBWall
from sailfish_amd.subdomain import Subdomain2D, Subdomain3D
from tests import _scn_twin as tw

GRID = {2: sym.D2Q9, 3: sym.D3Q19}
DTYPE = {'single': np.float32, 'double': np.float64}
# six distinct non-zero couplings and three distinct relaxation times, so that no index mix-up can hide
PARAMS = dict(G11=-0.31, G12=0.92, G13=0.73, G22=-0.27, G23=1.04, G33=-0.18, visc=0.09, tau_phi=0.87, tau_theta=1.21)


def couplings(p):
    return [[p['G11'], p['G12'], p['G13']], [p['G12'], p['G22'], p['G23']], [p['G13'], p['G23'], p['G33']]]


def global_fields(gshape, seed=7, amplitude=0.02):
    """rho, phi, theta on the global grid (numpy axis order): positive everywhere, around 1.0 / 0.7 / 0.5.  Defined on the
    global grid so that every decomposition starts from the same state."""
    rng = np.random.RandomState(seed)
    return [base + amplitude * rng.rand(*gshape) for base in (1.0, 0.7, 0.5)]


def solid(dim, h, gy, wall=4):
    """Slabs on both faces of y plus a block in the channel (as tests/_sc.make_wall_sim); h: global (x, y[, z])."""
    hx, hy = h[0], h[1]
    s = (hy < wall) | (hy >= gy - wall)
    block = (hx >= 5) & (hx < 9) & (hy >= wall + 2) & (hy < wall + 6)
    if dim == 3:
        block = block & (h[2] >= 1) & (h[2] < 5)
    return s | block


def make_sim(dim, walls=False, forces=None, seed=7):
    """forces: {lattice: acceleration} or None."""
    base = Subdomain2D if dim == 2 else Subdomain3D

    class Box(base):
        def boundary_conditions(self, *h):
            if walls:
                self.set_node(solid(dim, h, self.gy), NTFullBBWall)

        def initial_conditions(self, sim, *h):
            gshape = (self.gy, self.gx) if dim == 2 else (self.gz, self.gy, self.gx)
            where = tuple(reversed(h))
            for name, a in zip(('rho', 'phi', 'theta'), global_fields(gshape, seed)):
                getattr(sim, name)[:] = a[where]

    class Sim(LBTernaryFluidShanChen):
        subdomain = Box

        def __init__(self, config):
            super(Sim, self).__init__(config)
            for lattice, a in sorted((forces or {}).items()):
                self.add_body_force(tuple(a), grid=lattice)

    return Sim, (LBGeometry2D if dim == 2 else LBGeometry3D)


def config(dim, size, pattern='AB', fused=True, precision='double', potential='linear', force='guo', **over):
    cfg = dict(lat_nx=size[0], lat_ny=size[1], periodic_x=True, periodic_y=True, access_pattern=pattern,
               hip_fused_periodic=fused, precision=precision, grid=GRID[dim].__name__, sc_potential=potential,
               force_implementation=force, **PARAMS)
    if dim == 3:
        cfg.update(lat_nz=size[2], periodic_z=True)
    cfg.update(over)
    return cfg


def make_twin(dim, size, dtype, walls=False, forces=None, potential='linear', force='guo', seed=7, exp='libm', **over):
    grid = GRID[dim]
    shape = tuple(reversed(size))
    p = dict(PARAMS)
    p.update(over)
    wall = None
    if walls:
        idx = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
        wall = solid(dim, list(reversed(idx)), size[1])
    accel = [list((forces or {}).get(k, [0.0] * dim)) for k in range(3)]
    t = tw.ScTwin(grid, shape, dtype, [sym.relaxation_time(p['visc']), p['tau_phi'], p['tau_theta']], couplings(p),
                  potential=potential, accel=accel, edm=(force == 'edm'), wall=wall, exp=exp)
    zero = np.zeros(shape)
    t.set_fields(global_fields(shape, seed), [zero] * dim)
    return t


def merged(ctrl, what, grid_num=0):
    """A field ('rho', 'phi', 'theta', 'v0' ..) or the populations of a lattice ('dist') of every runner of `ctrl` on the
    global grid."""
    r0 = ctrl.runners[0]
    gshape = tuple(reversed(r0._global_size))
    out = np.zeros(((r0._sim.grid.Q,) if what == 'dist' else ()) + gshape, dtype=r0.float)
    for r in ctrl.runners:
        sp = r._spec
        sl = tuple(slice(o, o + n) for o, n in zip(reversed(sp.location), reversed(sp.size)))
        if what == 'dist':
            d = r._debug_get_dist(grid_num=grid_num)
            out[(slice(None),) + sl] = d[(slice(None),) + tuple(sp._nonghost_slice)]
        elif what[0] == 'v' and what[1:].isdigit():
            out[sl] = r._sim.v[int(what[1:])]
        else:
            out[sl] = getattr(r._sim, what)
    return out
