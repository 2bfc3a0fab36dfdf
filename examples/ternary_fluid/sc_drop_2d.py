#!/usr/bin/env python
"""Two resting drops in a ternary Shan-Chen mixture: a periodic D2Q9 box filled with component 1 (rho), one drop of
component 2 (phi) in the lower left and one of component 3 (theta) in the upper right.  Components 1 and 3 attract
themselves (G11 = G33 = -4.8, classic potential), which keeps the interfaces sharp; visc = 1/6.  Same defaults and
initial state as sailfish's examples/ternary_fluid/sc_drop_2d.py at its 256 x 256 size; the drops' radius is an eighth of
the box, so smaller boxes keep the picture.

    python examples/ternary_fluid/sc_drop_2d.py --max_iters=20000 [--profile_every=5000]

With --profile_every=N and matplotlib installed, the three densities along the box diagonal are drawn into
sc_drop_profiles.png every N steps."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np

from sailfish.controller import LBSimulationController
from sailfish.geo import LBGeometry2D
from sailfish.lb_ternary import LBTernaryFluidShanChen
from sailfish.subdomain import Subdomain2D

BULK = {'rho': 2.0, 'phi': 0.02, 'theta': 0.02}          # outside the drops
DROPS = [((0.25, 0.25), {'rho': 0.02, 'phi': 0.5, 'theta': 0.02}),
         ((0.75, 0.75), {'rho': 0.02, 'phi': 0.02, 'theta': 2.0})]


class DropSubdomain(Subdomain2D):
    def boundary_conditions(self, hx, hy):
        pass

    def initial_conditions(self, sim, hx, hy):
        radius = self.gx // 8
        for name, value in BULK.items():
            getattr(sim, name)[:] = value
        for (cx, cy), values in DROPS:
            inside = (hx - cx * self.gx) ** 2 + (hy - cy * self.gy) ** 2 <= radius ** 2
            for name, value in values.items():
                getattr(sim, name)[inside] = value


def draw_diagonal(sim, path):
    """rho, phi, theta along the diagonal of the box; returns False where matplotlib is missing."""
    try:
        import matplotlib
        matplotlib.use('Agg')
        from matplotlib import pyplot
    except ImportError:
        return False
    fig, ax = pyplot.subplots()
    for name, colour in (('rho', 'tab:red'), ('phi', 'tab:green'), ('theta', 'tab:blue')):
        field = np.asarray(getattr(sim, name), dtype=np.float64)
        ax.plot(np.diagonal(field), color=colour, label=name)
    ax.set_xlabel('node along the diagonal')
    ax.set_ylabel('density')
    ax.legend()
    fig.savefig(path)
    pyplot.close(fig)
    return True


class SCSim(LBTernaryFluidShanChen):
    subdomain = DropSubdomain

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--profile_every', type=int, default=0,
                           help='draw the density profiles along the diagonal every N steps (0: never)')

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'lat_nx': 256, 'lat_ny': 256, 'G11': -4.8, 'G33': -4.8, 'visc': 1.0 / 6.0, 'periodic_x': True,
                         'periodic_y': True, 'sc_potential': 'classic'})

    def after_step(self, runner):
        every = int(getattr(self.config, 'profile_every', 0) or 0)
        if every <= 0:
            return
        if (self.iteration + 1) % every == 0:
            self.need_sync_flag = True                    # the next step brings the fields to the host
        elif self.iteration % every == 0 and self.iteration > 0:
            draw_diagonal(runner._sim, 'sc_drop_profiles.png')


if __name__ == '__main__':
    LBSimulationController(SCSim, LBGeometry2D).run()
