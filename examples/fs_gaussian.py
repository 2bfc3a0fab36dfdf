#!/usr/bin/env python
"""A Gaussian hump of water spreading over a flat layer: the shallow-water model, D2Q9 (cf. sailfish's
examples/fs_gaussian.py; the same command line and defaults: a 62 x 62 box, visc 0.005, --gravity 0.001).

`rho` is the water depth: 1 far from the hump, 1.4 on top of it.  The hump collapses into a ring that travels outwards at
about sqrt(gravity h); with --periodic_x --periodic_y the ring leaves through one side and comes back through the other,
without them it meets the unconnected faces of the box.  The model conserves the water volume.

--bed_slope=S puts the layer on a periodic bed z_b(x) = -(S L / 2 pi) cos(2 pi x / L), L the box length along x, whose steepest
slope is S: the acceleration -gravity dz_b/dx = -gravity S sin(2 pi x / L) is a body force that depends on position
(LBForcedSim, a DynamicValue of S.gx), which the sweep reads as a field.  It needs --periodic_x to make
sense.  The plain force is not a well-balanced scheme: a lake at rest over such a bed, h + z_b = const, keeps a small
spurious current instead of staying exactly still."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root (the `sailfish` alias)

from sailfish.controller import LBSimulationController
from sailfish.geo import LBGeometry2D
from sailfish.lb_base import LBForcedSim
from sailfish.lb_single import LBFreeSurface
from sailfish.node_type import DynamicValue
from sailfish.subdomain import Subdomain2D
from sailfish.sym import S


class HumpSubdomain(Subdomain2D):
    amplitude = 0.4

    def boundary_conditions(self, hx, hy):
        pass

    def initial_conditions(self, sim, hx, hy):
        width = min(self.gx, self.gy) / 12.0
        r2 = (hx - self.gx / 2.0) ** 2 + (hy - self.gy / 2.0) ** 2
        sim.rho[:] = 1.0 + self.amplitude * np.exp(-r2 / width ** 2)


class HumpSim(LBFreeSurface, LBForcedSim):
    subdomain = HumpSubdomain

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'lat_nx': 62, 'lat_ny': 62, 'every': 10, 'visc': 0.005})

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--bed_slope', type=float, default=0.0,
                           help='steepest slope of a periodic cosine bed along x (0: flat bed, no body force)')

    def __init__(self, config):
        super(HumpSim, self).__init__(config)
        if config.bed_slope != 0.0:
            from sympy import sin
            k = 2.0 * math.pi / config.lat_nx
            self.add_body_force(DynamicValue(-config.gravity * config.bed_slope * sin(k * S.gx), 0.0))


if __name__ == '__main__':
    LBSimulationController(HumpSim, LBGeometry2D).run()
