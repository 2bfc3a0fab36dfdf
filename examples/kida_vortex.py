#!/usr/bin/env python
"""Decaying Kida vortex in a periodic box (the flow of sailfish's examples/turbulence/kida_vortex.py; S. Kida and
Y. Murakami, Kolmogorov similarity in freely decaying turbulence, Phys. Fluids 30, 2030 (1987)).  --grid chooses the
lattice: D3Q19 (the default here), D3Q15 (the reference's default for this flow) or D3Q27.  Kinetic energy and enstrophy
per node are formed on the device every --stats_every steps (20; sailfish.stats.KineticEnergyEnstrophyMixIn) and written
to <output>_ke_ens_<subdomain id>.dat as rows of (iteration, energy, enstrophy); without --output they go to the log.
--shift_x/y/z move the initial field by whole nodes: the statistics of a periodic box do not depend on them."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root (the `sailfish` alias)

import numpy as np

from sailfish.controller import LBSimulationController
from sailfish.geo import EqualSubdomainsGeometry3D
from sailfish.lb_single import LBFluidSim
from sailfish.stats import KineticEnergyEnstrophyMixIn
from sailfish.subdomain import Subdomain3D


def kida_velocity(x, y, z, max_v):
    """The Kida field at the phases x, y, z (each 0 .. 2 pi over the box); mean energy per node 3/8 max_v^2."""
    sin, cos = np.sin, np.cos
    return (max_v * sin(x) * (cos(3 * y) * cos(z) - cos(y) * cos(3 * z)),
            max_v * sin(y) * (cos(3 * z) * cos(x) - cos(z) * cos(3 * x)),
            max_v * sin(z) * (cos(3 * x) * cos(y) - cos(x) * cos(3 * y)))


class KidaSubdomain(Subdomain3D):
    max_v = 0.05

    def boundary_conditions(self, hx, hy, hz):
        pass

    def initial_conditions(self, sim, hx, hy, hz):
        cfg = self.config
        sim.rho[:] = 1.0
        x = (hx + getattr(cfg, 'shift_x', 0)) * np.pi * 2.0 / self.gx
        y = (hy + getattr(cfg, 'shift_y', 0)) * np.pi * 2.0 / self.gy
        z = (hz + getattr(cfg, 'shift_z', 0)) * np.pi * 2.0 / self.gz
        sim.vx[:], sim.vy[:], sim.vz[:] = kida_velocity(x, y, z, self.max_v)


class KidaSim(LBFluidSim, KineticEnergyEnstrophyMixIn):
    subdomain = KidaSubdomain
    every = 20          # steps between two samples

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'periodic_x': True, 'periodic_y': True, 'periodic_z': True,
                         'lat_nx': 110, 'lat_ny': 110, 'lat_nz': 110, 'grid': 'D3Q19',
                         'visc': 0.001375, 'access_pattern': 'AA', 'perf_stats_every': 200})

    @classmethod
    def add_options(cls, group, dim):
        # whole-node shifts of the initial field: the statistics must not depend on them
        group.add_argument('--shift_x', type=int, default=0)
        group.add_argument('--shift_y', type=int, default=0)
        group.add_argument('--shift_z', type=int, default=0)
        group.add_argument('--stats_every', type=int, default=0, help='steps between two samples (0: %d)' % cls.every)

    @classmethod
    def modify_config(cls, config):
        if not config.quiet:
            print('Re = {0}'.format(config.lat_nx * cls.subdomain.max_v / config.visc))

    def __init__(self, config):
        super(KidaSim, self).__init__(config)
        self.every = getattr(config, 'stats_every', 0) or type(self).every
        self.stats = []

    def after_step(self, runner):
        mod = self.iteration % self.every
        if mod == self.every - 1:
            self.need_fields_flag = True        # the next step stores the fields the sample reads
        elif mod == 0:
            ke, ens = self.compute_ke_enstropy(runner)
            self.stats.append((self.iteration, ke, ens))
            if self.config.output:
                np.savetxt('%s_ke_ens_%s.dat' % (self.config.output, runner._spec.id), np.array(self.stats))
            else:
                self.config.logger.info('iteration %d: kinetic energy %.9e, enstrophy %.9e' % (self.iteration, ke, ens))


if __name__ == '__main__':
    LBSimulationController(KidaSim, EqualSubdomainsGeometry3D).run()
