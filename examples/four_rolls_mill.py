#!/usr/bin/env python
"""The four-rolls mill, D2Q9 (cf. sailfish's examples/four_rolls_mill.py): the vortices of examples/taylor_green_2d.py held
steady by a body force that depends on position,

    a = visc k^2 u(x, y, t = 0),

which replaces exactly what viscosity takes out of them -- the initial state is the steady solution, and the printed
velocity error measures what the discretisation (and the forcing scheme) adds.  The force is a DynamicValue of S.gx, S.gy:
the host evaluates it once per node, in double precision at global coordinates, and the sweep reads it as a field
(DESIGN.md §9g)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root (the `sailfish` alias)

from sailfish.controller import LBSimulationController
from sailfish.geo import EqualSubdomainsGeometry2D
from sailfish.lb_base import LBForcedSim
from sailfish.node_type import DynamicValue
from sailfish.sym import S

from examples.taylor_green_2d import TaylorGreenSim, TaylorGreenSubdomain


class FourRollsMill(TaylorGreenSim, LBForcedSim):
    def reference_solution(self, hx, hy, nx, ny, iteration, Ma):
        return self.subdomain.solution(self.config, hx, hy, nx, ny, 0, Ma)       # steady: the state at t = 0

    def __init__(self, config):
        super(FourRollsMill, self).__init__(config)
        from sympy import cos, sin
        kx, ky, ksq, k = TaylorGreenSubdomain.get_k(config, config.lat_nx, config.lat_ny)
        amp = config.visc * ksq * config.max_v / k
        self.add_body_force(DynamicValue(-amp * ky * sin(ky * S.gy) * cos(kx * S.gx),
                                         amp * kx * sin(kx * S.gx) * cos(ky * S.gy)))


if __name__ == '__main__':
    LBSimulationController(FourRollsMill, EqualSubdomainsGeometry2D).run()
