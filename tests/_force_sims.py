"""Simulations of the force-object tests (tests/test_force_objects.py on the CPU, tests/test_gpu_force_objects.py on the
GPU): the cylinder channel of examples/cylinder.py and the sphere duct of examples/sphere_3d.py, each with an active-node
map for indirect addressing (solid nodes without a fluid neighbour own no slot) and the given force objects.  Test-only."""
import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish.lb_base import ForceObject

from tests import _host

# lattice sizes and an interior box around the body (no link of it leaves the domain)
CYLINDER = dict(lat_nx=48, lat_ny=30, visc=0.1, vertical=False, force_implementation='guo')
CYLINDER_BOX = ((13, 8), (27, 22))
SPHERE = dict(lat_nx=20, lat_ny=16, lat_nz=16, visc=0.05, grid='D3Q19', force_implementation='guo')
SPHERE_BOX = ((6, 4, 4), (15, 12, 12))


def cylinder_sim(boxes=(CYLINDER_BOX,), hook=None):
    """CylinderSim with a ForceObject per (start, end) of `boxes`; hook(sim, runner) runs after every step."""
    base = _host.load_sim_class('cylinder', 'CylinderSimulation')

    class Sub(base.subdomain):
        def load_active_node_map(self, hx, hy):
            d = self.gy / 3
            inside = (hx - 2 * d) ** 2 + (hy - self.gy / 2) ** 2 < d ** 2 / 4.0
            self.set_active_node_map_from_wall_map((hy <= 0) | (hy >= self.gy - 1) | inside)

    return _with_objects(base, Sub, boxes, hook)


def sphere_sim(boxes=(SPHERE_BOX,), hook=None):
    base = _host.load_sim_class('sphere_3d', 'SphereSimulation')

    class Sub(base.subdomain):
        def load_active_node_map(self, hx, hy, hz):
            d = self.gy / 3.0
            r2 = (hx - 2.0 * d) ** 2 + (hy - self.gy / 2.0) ** 2 + (hz - self.gz / 2.0) ** 2
            duct = (hy <= 0) | (hy >= self.gy - 1) | (hz <= 0) | (hz >= self.gz - 1)
            self.set_active_node_map_from_wall_map(duct | (r2 <= (d / 2.0) ** 2))

    return _with_objects(base, Sub, boxes, hook)


def _with_objects(base, sub, boxes, hook):
    class Sim(base):
        subdomain = sub

        def __init__(self, config):
            super(Sim, self).__init__(config)
            for start, end in boxes:
                self.add_force_oject(ForceObject(start, end))

        if hook is not None:
            def after_step(self, runner):
                hook(self, runner)

    return Sim
