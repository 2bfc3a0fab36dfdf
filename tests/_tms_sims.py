"""The duct of tests/test_gpu_tms.py's indirect-addressing cases; test-only.  Tamm-Mott-Smith walls on the four rims normal
to y and z, x periodic, a body force along x, and a block of full-way bounce-back nodes in the middle whose innermost node
has no fluid neighbour and owns no slot, so that slots and dense indices differ.  The wall map handed to
set_active_node_map_from_wall_map() names the block only: TMS nodes are wet, and the layer of ghost nodes behind them --
where their even in-place step stores what it reflects -- stays active.

Run as a script it is the child process of test_indirect_addressing_per_node_kernel (the library reads
SLF_INDIRECT_SLOTS once per process): <output directory> -> <pattern>.<field>.npy of the indirect runs."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish import node_type as nt
from sailfish.lb_base import LBForcedSim
from sailfish.lb_single import LBFluidSim
from sailfish.subdomain import Subdomain3D

CFG = dict(lat_nx=20, lat_ny=10, lat_nz=9, grid='D3Q19', visc=0.05, periodic_x=True, force_implementation='guo',
           model='bgk')
STEPS = 21


class DuctSubdomain(Subdomain3D):
    def _block(self, hx, hy, hz):
        return (np.abs(hx - self.gx // 2) <= 1) & (np.abs(hy - self.gy // 2) <= 1) & (np.abs(hz - self.gz // 2) <= 1)

    def boundary_conditions(self, hx, hy, hz):
        self.set_node((hy == 0) | (hy == self.gy - 1) | (hz == 0) | (hz == self.gz - 1), nt.NTWallTMS)
        self.set_node(self._block(hx, hy, hz), nt.NTFullBBWall)

    def initial_conditions(self, sim, hx, hy, hz):
        sim.rho[:] = 1.0 + 0.01 * np.sin(2 * np.pi * hx / self.gx)
        sim.vx[:] = 0.02
        sim.vy[:] = 0.01 * np.cos(2 * np.pi * hx / self.gx)

    def load_active_node_map(self, hx, hy, hz):
        self.set_active_node_map_from_wall_map(self._block(hx, hy, hz))


class DuctSim(LBFluidSim, LBForcedSim):
    subdomain = DuctSubdomain

    def __init__(self, config):
        super(DuctSim, self).__init__(config)
        self.add_body_force((1e-5, 0.0, 0.0))


class DuctSimNoForce(LBFluidSim):
    subdomain = DuctSubdomain


if __name__ == '__main__':
    from tests.test_gpu_runner import merged_gpu, run_gpu
    out_dir = sys.argv[1]
    print('SLF_INDIRECT_SLOTS=%s' % os.environ.get('SLF_INDIRECT_SLOTS'), flush=True)
    for pattern in ('AB', 'AA'):
        ctrl = run_gpu(DuctSim, None, 3, dict(CFG, access_pattern=pattern, precision='single', node_addressing='indirect'),
                       STEPS)
        assert all(r._desc.node_addressing == 1 for r in ctrl.runners)
        np.save(os.path.join(out_dir, '%s.rho.npy' % pattern), merged_gpu(ctrl, 'rho'))
        for d in range(3):
            np.save(os.path.join(out_dir, '%s.v%d.npy' % (pattern, d)), merged_gpu(ctrl, 'v%d' % d))
        for r in ctrl.runners:
            r.release()
        print('done', pattern, flush=True)
