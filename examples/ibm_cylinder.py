#!/usr/bin/env python
"""Flow past a cylinder made of immersed boundary markers (2-D).

Fifty markers sit on a circle of radius 10 a quarter of the way down a 512 x 128 channel.  Every marker is tied to its
starting point by a spring; the spring forces are spread onto the four nodes around each marker and enter the collision as
a body force, and the markers follow the interpolated fluid velocity (LBIBMFluidSim).  The channel has
full-way bounce-back walls at the top and bottom, a velocity inlet on the left and a copying outlet on the right, and a
uniform body force drives the flow at a Reynolds number of 150 with respect to the diameter, where a cylinder sheds
vortices (Strouhal number about 0.18).  Every 20 steps the velocity at a probe three quarters down the centreline is
printed: iteration, vy, vx.  The shedding frequency is the strongest peak of the spectrum of vy once the flow has settled.

    python examples/ibm_cylinder.py --max_iters=2000
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root (the `sailfish` alias)

from sailfish.controller import LBSimulationController
from sailfish.lb_single import LBIBMFluidSim, Particle
from sailfish.node_type import NTCopy, NTFullBBWall, NTRegularizedVelocity
from sailfish.subdomain import Subdomain2D

RADIUS = 10
MARKERS = 50
REYNOLDS = 150
STIFFNESS = 0.01
INLET_VELOCITY = (0.03, 0.0)
PROBE_EVERY = 20


class CylinderSubdomain(Subdomain2D):
    def boundary_conditions(self, hx, hy):
        walls = (hy == 0) | (hy == self.gy - 1)
        self.set_node(walls, NTFullBBWall)
        self.set_node(~walls & (hx == 0), NTRegularizedVelocity(INLET_VELOCITY))
        self.set_node(~walls & (hx == self.gx - 1), NTCopy)

    def initial_conditions(self, sim, hx, hy):
        sim.rho[:] = 1.0
        sim.vx[:] = 0.0
        sim.vy[:] = 0.0
        centre = (0.25 * self.config.lat_nx, 0.5 * self.config.lat_ny)
        for i in range(MARKERS):
            angle = 2.0 * math.pi * i / float(MARKERS)
            at = (centre[0] + RADIUS * math.cos(angle), centre[1] + RADIUS * math.sin(angle))
            sim.add_particle(Particle(at, stiffness=STIFFNESS, ref_position=at))


class CylinderSimulation(LBIBMFluidSim):
    subdomain = CylinderSubdomain

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'lat_nx': 512, 'lat_ny': 128, 'visc': 0.01, 'perf_stats_every': 500})

    def __init__(self, config):
        super(CylinderSimulation, self).__init__(config)
        diameter = 2 * RADIUS
        max_v = REYNOLDS / float(diameter) * config.visc
        # the force that drives a plane Poiseuille flow of width `diameter` to max_v
        force = 8.0 * config.visc * max_v / diameter ** 2
        self.add_body_force((force, 0.0))
        self.config.logger.info('v_max:%.3e  Re:%d  F:%.3e' % (max_v, REYNOLDS, force))

    def after_step(self, runner):
        phase = self.iteration % PROBE_EVERY
        if phase == PROBE_EVERY - 1:
            self.need_sync_flag = True               # the fields of the coming step are copied to the host
        elif phase == 0:
            y, x = self.config.lat_ny // 2, (3 * self.config.lat_nx) // 4
            print(self.iteration, self.vy[y, x], self.vx[y, x])


if __name__ == '__main__':
    LBSimulationController(CylinderSimulation).run()
