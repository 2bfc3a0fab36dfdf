#!/usr/bin/env python
"""Rayleigh-Benard convection (2-D): a layer of fluid heated from below.

The box is periodic along x and closed by full-way bounce-back walls at the bottom (wall_temperature = 1) and at the top
(wall_temperature = 0); gravity points down, so the buoyancy b (T - 1/2) points up (LBThermalFluidSim).
--Ra and --Pr set the Rayleigh and Prandtl numbers: the diffusivity is visc / Pr and b = Ra visc kappa / H^3 with H the
distance between the wall mid-points (lat_ny - 2) and a temperature difference of 1.  The fluid starts at rest on the
conduction profile plus a small sinusoidal perturbation.  Below Ra = 1707.76 the perturbation dies; above it convection
rolls grow until the heat they carry balances the driving.  Every --every steps the kinetic energy of the fluid and the
Nusselt number 1 + <v_y T> H / kappa (the volume average over the fluid) are printed: iteration, energy, Nu.

    python examples/rayleigh_benard_2d.py --Ra=5000 --max_iters=20000 --every=500
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root (the `sailfish` alias)

from sailfish.controller import LBSimulationController
from sailfish.lb_thermal import LBThermalFluidSim
from sailfish.node_type import NTFullBBWall
from sailfish.subdomain import Subdomain2D

PERTURBATION = 1e-3


class LayerSubdomain(Subdomain2D):
    def boundary_conditions(self, hx, hy):
        self.set_node((hy == 0) | (hy == self.gy - 1), NTFullBBWall)

    def initial_conditions(self, sim, hx, hy):
        H = float(self.gy - 2)
        sim.rho[:] = 1.0
        sim.vx[:] = 0.0
        sim.vy[:] = 0.0
        sim.T[:] = 1.0 - (hy - 0.5) / H + PERTURBATION * np.sin(2.0 * np.pi * hx / self.gx) * np.sin(np.pi * (hy - 0.5) / H)
        sim.wall_temperature[hy == 0] = 1.0
        sim.wall_temperature[hy == self.gy - 1] = 0.0


class RayleighBenardSimulation(LBThermalFluidSim):
    subdomain = LayerSubdomain

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--Ra', type=float, default=5000.0, help='Rayleigh number')
        group.add_argument('--Pr', type=float, default=1.0, help='Prandtl number (visc / thermal diffusivity)')

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'lat_nx': 128, 'lat_ny': 66, 'visc': 0.03, 'periodic_x': True, 'every': 500, 'perf_stats_every': 5000})

    @classmethod
    def modify_config(cls, config):
        config.thermal_diffusivity = config.visc / getattr(config, 'Pr', 1.0)

    def __init__(self, config):
        super(RayleighBenardSimulation, self).__init__(config)
        H = float(config.lat_ny - 2)
        self.buoyancy_strength = getattr(config, 'Ra', 5000.0) * config.visc * config.thermal_diffusivity / H ** 3
        self.set_buoyancy((0.0, self.buoyancy_strength), t_ref=0.5)

    def after_step(self, runner):
        every = max(1, int(self.config.every))
        phase = self.iteration % every
        if phase == every - 1:
            self.need_sync_flag = True               # the fields of the coming step are copied to the host
        elif phase == 0:
            fluid = slice(1, -1)                     # the rows between the walls
            vx, vy, T = self.vx[fluid].astype(np.float64), self.vy[fluid].astype(np.float64), self.T[fluid].astype(np.float64)
            H = float(self.config.lat_ny - 2)
            energy = 0.5 * (vx ** 2 + vy ** 2).sum()
            nusselt = 1.0 + (vy * T).mean() * H / self.config.thermal_diffusivity
            print(self.iteration, energy, nusselt)


if __name__ == '__main__':
    LBSimulationController(RayleighBenardSimulation).run()
