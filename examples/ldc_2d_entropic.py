#!/usr/bin/env python
"""Lid-driven cavity at Re = 7500 on 126 x 126 nodes with the entropic collision (--model=elbm): the resolution is far
too low for plain BGK at this Reynolds number; the entropic model picks, node by node, the relaxation alpha that keeps
the entropy from growing.  The geometry is that of examples/ldc_2d.py with a slower lid.

The simulation class is LBEntropicFluidSim: besides rho and v it carries the field `alpha`, which goes to the output
files like any other field (alpha = 2: resolved; < 2: smoothed; > 2: enhanced) and into checkpoints.

    python examples/ldc_2d_entropic.py --max_iters=20000 --every=2000 --output=/tmp/ldc_entropic
    python examples/ldc_2d_entropic.py --entropic_equilibrium ...     # the product-form equilibrium

The same example of sailfish-team/sailfish also outputs an `entropy` field, computed by a kernel the user supplies as
source text (ComputeEntropy in entropic_utils.mako).  This backend runs a pre-built library and cannot take user
kernels, so that field is not offered; H = sum_i f_i ln(f_i / w_i) can be formed on the host from a dump of the
populations (--debug_dump_dists).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root (the `sailfish` alias)

from sailfish.controller import LBSimulationController
from sailfish.lb_single import LBEntropicFluidSim

from examples.ldc_2d import CavitySubdomain


class SlowLidSubdomain(CavitySubdomain):
    lid_velocity = 0.01


class EntropicCavitySim(LBEntropicFluidSim):
    subdomain = SlowLidSubdomain

    @classmethod
    def update_defaults(cls, defaults):
        n = 126
        defaults.update({'model': 'elbm', 'lat_nx': n, 'lat_ny': n,
                         'visc': (n - 2) * SlowLidSubdomain.lid_velocity / 7500.0})


if __name__ == '__main__':
    LBSimulationController(EntropicCavitySim).run()
