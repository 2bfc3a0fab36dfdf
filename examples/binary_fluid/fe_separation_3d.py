#!/usr/bin/env python
"""Spinodal decomposition of a binary fluid with the free-energy model in a periodic D3Q19 box (the set-up of sailfish's
examples/binary_fluid/fe_separation_3d.py: 32^3, kappa = 2e-4, A = 1e-4, Gamma = 25, tau_a = 4.5, tau_b = 0.8, rho = 1 and
an order parameter of U[0, 0.01))."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np

from sailfish.controller import LBSimulationController
from sailfish.geo import LBGeometry3D
from sailfish.lb_binary import LBBinaryFluidFreeEnergy
from sailfish.subdomain import Subdomain3D


class SeparationSubdomain(Subdomain3D):
    def boundary_conditions(self, hx, hy, hz):
        pass

    def initial_conditions(self, sim, hx, hy, hz):
        # noise on the global grid: every decomposition starts from the same state
        noise = np.random.RandomState(self.config.seed).rand(self.gz, self.gy, self.gx) / 100.0
        sim.rho[:] = 1.0
        sim.phi[:] = noise[hz, hy, hx]


class SeparationFESim(LBBinaryFluidFreeEnergy):
    subdomain = SeparationSubdomain

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'lat_nx': 32, 'lat_ny': 32, 'lat_nz': 32, 'grid': 'D3Q19', 'kappa': 2e-4, 'Gamma': 25.0,
                         'A': 1e-4, 'tau_a': 4.5, 'tau_b': 0.8, 'tau_phi': 1.0, 'periodic_x': True, 'periodic_y': True,
                         'periodic_z': True})


if __name__ == '__main__':
    LBSimulationController(SeparationFESim, LBGeometry3D).run()
