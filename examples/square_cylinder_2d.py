#!/usr/bin/env python
"""Flow past a square cylinder in a plane channel, D2Q9, with the drag and lift on the cylinder measured by momentum
exchange (cf. sailfish's examples/square_cylinder_2d.py; the case of Breuer, Bernsdorf, Zeiser, Durst, Int. J. Heat Fluid
Flow 21 (2000) 186-196: channel height H, length 6.25 H, cylinder edge D = H / 8 a quarter of the length downstream).

The inlet prescribes the developed parabolic profile with peak velocity MAX_V as a DynamicValue of the node position, the
outlet a constant density; channel walls and cylinder are half-way (default) or full-way bounce-back nodes.  A
ForceObject whose box surrounds the cylinder gives the force on it; every --every steps the script prints

    iteration  F_x  F_y  C_D  C_L            C = 2 F / (D MAX_V^2)

and stops once neither component has changed by more than --settled (relative) between two samples."""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root (the `sailfish` alias)

import numpy as np

from sailfish.controller import LBSimulationController
from sailfish.lb_base import ForceObject
from sailfish.lb_single import LBFluidSim
from sailfish.node_type import DynamicValue, NTEquilibriumDensity, NTEquilibriumVelocity, NTFullBBWall, NTHalfBBWall
from sailfish.subdomain import Subdomain2D
from sailfish.sym import S

MAX_V = 0.025
WALLS = {'halfbb': NTHalfBBWall, 'fullbb': NTFullBBWall}


def geometry(config):
    """(H, L, D, wall type): channel height between the walls, channel length, cylinder edge -- all in node spacings."""
    H = int(config.H)
    L = int(6.25 * H)
    return H, L, int(0.02 * L), WALLS[config.wall]


def profile(across, H):
    """Developed channel flow: `across` = distance from the lower wall."""
    return 4.0 * MAX_V / H ** 2 * across * (H - across)


class CylinderSubdomain(Subdomain2D):
    def boundary_conditions(self, hx, hy):
        H, L, D, wall = geometry(self.config)
        walls = (hy == 0) | (hy == self.gy - 1)
        self.set_node(walls, wall)
        # the wall sits wall.location node spacings off the outermost node layer (half-way: outside it, full-way: inside)
        self.set_node((hx == 0) & ~walls, NTEquilibriumVelocity(DynamicValue(profile(S.gy - wall.location, H), 0.0)))
        self.set_node((hx == self.gx - 1) & ~walls, NTEquilibriumDensity(1.0))
        # node layers that make a cylinder of edge D: full-way bounce-back walls sit half a spacing outside their nodes,
        # half-way ones inside
        layers = D - 1 if wall.location == 0.5 else D + 2
        x0 = int(math.floor(L / 4.0 - (layers - 1) / 2.0 + 0.5))
        y0 = int(math.floor((self.gy - 1) / 2.0 - (layers - 1) / 2.0 + 0.5))
        self.set_node((hx >= x0) & (hx < x0 + layers) & (hy >= y0) & (hy < y0 + layers), wall)

    def initial_conditions(self, sim, hx, hy):
        H, _, _, wall = geometry(self.config)
        sim.rho[:] = 1.0
        sim.vy[:] = 0.0
        sim.vx[:] = profile(hy - wall.location, H)


class SquareCylinderSim(LBFluidSim):
    subdomain = CylinderSubdomain

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--H', type=int, default=80, help='channel height in node spacings (length 6.25 H, cylinder H / 8)')
        group.add_argument('--wall', type=str, choices=sorted(WALLS), default='halfbb', help='channel walls and cylinder')
        group.add_argument('--force_every', type=int, default=500, help='steps between two samples of the force')
        group.add_argument('--settled', type=float, default=1e-6,
                           help='stop when no force component changed by more than this (relative) between two samples')

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'precision': 'double', 'max_iters': 1000000, 'visc': 0.05})

    @classmethod
    def modify_config(cls, config):
        H, L, _, wall = geometry(config)
        config.lat_nx = L
        config.lat_ny = H + 2 if wall.location == 0.5 else H

    def __init__(self, config):
        super(SquareCylinderSim, self).__init__(config)
        H, L, D, _ = geometry(config)
        self.D = D
        margin = 5
        self.add_force_oject(ForceObject((L / 4.0 - D / 2.0 - margin, (config.lat_ny - D) / 2.0 - margin),
                                         (L / 4.0 + D / 2.0 + margin, (config.lat_ny + D) / 2.0 + margin)))
        self.samples = []           # (iteration, F_x, F_y, C_D, C_L)
        if not getattr(config, 'quiet', False):
            print('%d x %d | cylinder: %d | Re = %.1f' % (L, H, D, MAX_V * D / config.visc))

    def record_value(self, iteration, force, C_D, C_L):
        self.samples.append((iteration, force[0], force[1], C_D, C_L))
        if not getattr(self.config, 'quiet', False):
            print(iteration, force[0], force[1], C_D, C_L)

    def after_step(self, runner):
        if self.iteration % self.config.force_every:
            return
        runner.update_force_objects()
        for fo in self.force_objects:
            if not fo.initialized:          # (this subdomain holds no part of the cylinder)
                continue
            runner.backend.from_buf(fo.gpu_force_buf)
            f = np.array(fo.force())
            scale = 2.0 / (self.D * MAX_V ** 2)
            previous = self.samples[-1][1:3] if self.samples else None
            self.record_value(self.iteration, f, scale * f[0], scale * f[1])
            if previous is not None and np.all(np.abs(f - previous) <= self.config.settled * np.abs(f)):
                runner._quit_event.set()        # steady state


if __name__ == '__main__':
    LBSimulationController(SquareCylinderSim).run()
