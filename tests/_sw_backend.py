"""The CPU test backend (tests/_oracle_backend.py) with the numpy twin of the shallow-water model (tests/_sw_twin.py) behind
CollideAndPropagate and SetInitialConditions of a module built with equilibrium = SLF_EQ_SHALLOW_WATER, so that the
product's host stack -- controller, runner, halo exchange, step plans -- runs LBFreeSurface on a machine without a GPU.
The other kernels (ghost-layer periodicity, index-list and face copies) move data and stay the oracle's; a module with the
polynomial is the oracle's altogether.  It has the acceleration-field call of backend_hip.HIPBackend and records, as
tests/_accf_backend.py does: LOG holds ('build', equilibrium, gravity), ('set_accel_field', module, address, host copy),
('get_kernel', name) and ('run', name) in call order.  Selected with backends='tests._sw_backend'.  Test-only."""
import ctypes

import numpy as np

from sailfish_amd import hipabi
from tests import _sw_twin as tw
from tests._oracle_backend import OracleBackend

LOG = []


def _array(addr, dtype, shape):
    n = int(np.prod(shape))
    raw = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(int(addr))
    return np.frombuffer(raw, dtype=dtype, count=n).reshape(shape)


class SwTwinBackend(OracleBackend):
    name = 'oracle_sw_test'

    @classmethod
    def add_options(cls, group):
        group.add_argument('--nohip_accel_field', dest='hip_accel_field', action='store_false', default=True)
        return OracleBackend.add_options(group)

    def build(self, source):
        LOG.append(('build', int(source.equilibrium), float(source.gravity)))
        m = super(SwTwinBackend, self).build(source)
        m.twin = tw.SwTwin(source) if int(source.equilibrium) == hipabi.SLF_EQ_SHALLOW_WATER else None
        return m

    def _views(self, module):
        d = module.desc
        dtype = np.float32 if d.precision == 4 else np.float64
        shape = (d.arr_nz, d.arr_ny, d.arr_nx)
        n, stride = int(np.prod(shape)), hipabi.dist_stride(d)
        dist = lambda a: _array(a, dtype, (9, stride))[:, :n].reshape((9,) + shape)       # noqa: E731
        field = lambda a: _array(a, dtype, shape)                                           # noqa: E731
        return dtype, shape, dist, field

    def set_accel_field(self, module, buf):
        d = module.desc
        dtype, shape, _, _ = self._views(module)
        field = _array(buf, dtype, (2,) + shape)
        LOG.append(('set_accel_field', module, int(buf), field.copy()))
        if module.twin is not None:
            module.twin.set_accel_field(field)          # a view: the runner's buffer

    def get_kernel(self, prog, name, *args, **kw):
        LOG.append(('get_kernel', name))
        return super(SwTwinBackend, self).get_kernel(prog, name, *args, **kw)

    def run_kernel(self, k, grid_size=None, stream=None):
        LOG.append(('run', k.name))
        m = k.module
        if m.twin is None or k.name not in ('CollideAndPropagate', 'SetInitialConditions'):
            return super(SwTwinBackend, self).run_kernel(k, grid_size, stream)
        d, a = m.desc, k.args
        _, shape, dist, field = self._views(m)
        if k.name == 'SetInitialConditions':            # dist, vx, vy, rho, map
            m.twin.init(dist(a[0]), field(a[3]), field(a[1]), field(a[2]))
            return
        nmap = _array(a[0], np.uint32, shape) if a[0] else None
        prop = (2 if (k.iteration & 1) else 1) if d.access_pattern == hipabi.SLF_AA else 0
        region = None if grid_size is None else tuple(int(v) for v in grid_size)
        m.twin.step(prop, nmap, dist(a[1]), dist(a[2]), field(a[3]), field(a[4]), field(a[5]), None, a[6], region)


backend = SwTwinBackend
