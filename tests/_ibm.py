"""Set-ups shared by the tests of the immersed boundary markers (tests/test_gpu_ibm.py, tests/test_ibm_host.py): the marker
sets of the parity tests, the channel simulation with a ring of markers, the box-level step.  Test-only."""
import math

import numpy as np

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish_amd.lb_single import LBIBMFluidSim, Particle
from sailfish_amd.node_type import NTFullBBWall
from sailfish_amd.subdomain import Subdomain2D, Subdomain3D

SHAPES = {'D2Q9': (32, 16), 'D3Q19': (16, 12, 10)}
N_MARKERS = 130              # one past a 128-lane workgroup


def marker_set(size, seed=11):
    """(position [130, dim], reference position, stiffness, index of the marker whose stencil leaves the real nodes).
    Global coordinates 0 .. size - 1 are the real nodes.  0, 1: two markers in one cell; 2: at integer coordinates;
    3: stencil beyond the last real column (x in (nx - 1, nx)); 4: next to the low y face (in the walled 2-D channel its
    stencil holds wall nodes, which are not wet); 5 .. 8 in 3-D: dz near 0.5, so that both z layers carry weight;
    10 .. 49: forty markers at one identical position; the rest scattered at least two nodes from every face."""
    dim = len(size)
    rng = np.random.RandomState(seed)
    hi = np.array(size, dtype=np.float64) - 3.0
    pos = 2.0 + rng.rand(N_MARKERS, dim) * (hi - 2.0)
    cell = np.floor(pos[0])
    pos[0] = cell + 0.25
    pos[1] = cell + np.array([0.75, 0.5, 0.125])[:dim]
    pos[2] = np.array([5.0, 4.0, 3.0])[:dim]
    pos[3, 0] = size[0] - 0.5
    pos[4, 1] = 0.375
    if dim == 3:
        pos[5:9, 2] = np.floor(pos[5:9, 2]) + np.array([0.5, 0.4999, 0.5001, 0.46875])
    pos[10:50] = pos[10]
    ref = pos + 0.6 * (rng.rand(N_MARKERS, dim) - 0.5)
    ref[2] = pos[2] + 0.25
    stiffness = 0.002 + 0.02 * rng.rand(N_MARKERS)
    return pos, ref, stiffness, 3


class BoxWithMarkers(object):
    """sailfish_amd.box.BoxSim with sailfish_amd.ibm.Markers around its step: the step sequence of tests/_ibm_twin.IbmTwinBox
    on the device."""

    def __init__(self, backend, desc, periodic, node_map, position, ref_position, stiffness, origin=(0, 0, 0)):
        from sailfish_amd import ibm
        from sailfish_amd.box import BoxSim
        dim = position.shape[1]
        shape = tuple(reversed([desc.lat_nx - 2, desc.lat_ny - 2] + ([desc.lat_nz - 2] if dim == 3 else [])))
        self.box = BoxSim(backend, desc, periodic=periodic, node_map=node_map, accel_field=np.zeros((dim,) + shape),
                          accel_field_fill=np.nan)
        self.backend, self.dim = backend, dim
        self.markers = ibm.Markers(backend, self.box.module, self.box.dtype, dim, origin, position, ref_position, stiffness)

    def front(self):
        self.markers.front(self.box.stream)

    def back(self):
        self.markers.back(self.box.gpu_map, self.box.gpu_v, self.box.stream)

    def step(self):
        self.front()
        self.box.step(save_macro=True)
        self.back()

    def field(self):
        self.box.sync()
        self.backend.from_buf(self.box.gpu_accel_field)
        return np.array(self.box.accel_field)

    def acc(self):
        self.box.sync()
        self.backend.from_buf(self.markers.gpu_acc)
        return np.array(self.markers.acc).reshape((self.dim,) + self.box.shape)

    def positions(self):
        return self.markers.positions(self.box.stream)

    def outside(self):
        return self.markers.outside_count(self.box.stream)

    def release(self):
        self.box.sync()
        self.markers.release()
        self.box.release()


def ring(centre, radius, n):
    return [(centre[0] + radius * math.cos(2.0 * math.pi * i / n), centre[1] + radius * math.sin(2.0 * math.pi * i / n))
            for i in range(n)]


def channel_sim(dim, positions, refs, stiffness, accel, walls=True, start=None):
    """LBIBMFluidSim in a box that is periodic along x (and z), between full-way walls on the y faces (walls=True), driven by
    the uniform acceleration `accel`, with the given markers.  start: None = fluid at rest, else (rho, v) on the global grid."""
    base = Subdomain2D if dim == 2 else Subdomain3D

    class Channel(base):
        def boundary_conditions(self, *h):
            if walls:
                self.set_node((h[1] == 0) | (h[1] == self.gy - 1), NTFullBBWall)

        def initial_conditions(self, sim, *h):
            sim.rho[:] = 1.0
            if start is not None:
                where = tuple(reversed(h))
                sim.rho[:] = start[0][where]
                for c, a in zip(sim.v, start[1]):
                    c[:] = a[where]
            for p, r, k in zip(positions, refs, stiffness):
                sim.add_particle(Particle(tuple(p), stiffness=float(k), ref_position=tuple(r)))

    class Sim(LBIBMFluidSim):
        subdomain = Channel

        def __init__(self, config):
            super(Sim, self).__init__(config)
            if accel is not None:
                self.add_body_force(tuple(accel))

    return Sim


def channel_cfg(size, pattern='AB', precision='single', model='bgk', visc=0.05, **over):
    cfg = dict(lat_nx=size[0], lat_ny=size[1], periodic_x=True, access_pattern=pattern, precision=precision, model=model,
               visc=visc)
    if len(size) == 3:
        cfg.update(lat_nz=size[2], periodic_z=True)
    cfg.update(over)
    return cfg
