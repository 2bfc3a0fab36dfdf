"""The CPU test backend (tests/_oracle_backend.py) with the force-object calls of backend_hip.HIPBackend: force_workspace()
and force_objects() on host memory, the sums by the numpy twin (tests/_force_twin.py).  Selected with
backends='tests._force_backend'.  Test-only."""
import ctypes

import numpy as np

from sailfish_amd import hipabi, sym
from tests import _force_twin
from tests._oracle_backend import OracleBackend


def _array(addr, dtype, count):
    buf = (ctypes.c_char * (int(count) * np.dtype(dtype).itemsize)).from_address(int(addr))
    return np.frombuffer(buf, dtype=dtype, count=int(count))


class ForceOracleBackend(OracleBackend):
    name = 'oracle_force_test'

    def force_workspace(self, module, n_objects, max_links):
        return 0

    def force_objects(self, module, gpu_dist, idx, idx2, dirs, seg, n_objects, max_links, workspace, out, stream=None):
        d = module.desc
        grid = sym.D2Q9 if d.lattice == hipabi.SLF_D2Q9 else sym.D3Q19
        dist = _array(gpu_dist, np.float32 if d.precision == 4 else np.float64, grid.Q * hipabi.dist_stride(d))
        seg = _array(seg, np.uint32, n_objects + 1)
        n = int(seg[-1])
        idx, idx2, dirs = _array(idx, np.uint32, n), _array(idx2, np.uint32, n), _array(dirs, np.uint8, n)
        res = _array(out, np.float64, 3 * n_objects)
        for o in range(n_objects):
            sl = slice(int(seg[o]), int(seg[o + 1]))
            assert sl.stop - sl.start <= max_links
            res[3 * o:3 * o + 3] = _force_twin.fsum_force(_force_twin.link_terms(dist, idx[sl], idx2[sl], dirs[sl], grid))


backend = ForceOracleBackend
