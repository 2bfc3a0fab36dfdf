"""The CPU test backend (tests/_oracle_backend.py) with the thermal calls of backend_hip.HIPBackend, recording what the runner
does with them: LOG holds ('build', accel_field), ('set_accel_field', address), ('thermal_init' | 'thermal_step', ...) and
('run', kernel name, options, stream) in call order.  The oracle behind it knows neither field nor temperature, so the numbers
of the fluid mean nothing; to make the populations and the field something a checkpoint can lose, thermal_step writes
g_dst = g_src + STEP and adds STEP to the field (exact in both formats).  Selected with backends='tests._thermal_backend'.
Test-only."""
import ctypes

import numpy as np

from tests._oracle_backend import OracleBackend

LOG = []
STEP = 0.125


class ThermalRecordingBackend(OracleBackend):
    name = 'oracle_thermal_test'
    supports_thermal = True

    @classmethod
    def add_options(cls, group):
        group.add_argument('--nohip_accel_field', dest='hip_accel_field', action='store_false', default=True)
        return OracleBackend.add_options(group)

    @staticmethod
    def _shape(module):
        d = module.desc
        dim = 2 if d.lattice == 0 else 3
        return dim, np.float32 if d.precision == 4 else np.float64, d.arr_nz * d.arr_ny * d.arr_nx

    @staticmethod
    def _view(addr, dtype, count):
        raw = (ctypes.c_char * (count * np.dtype(dtype).itemsize)).from_address(int(addr))
        return np.frombuffer(raw, dtype=dtype, count=count)

    def build(self, source):
        LOG.append(('build', int(source.accel_field)))
        return super(ThermalRecordingBackend, self).build(source)

    def set_accel_field(self, module, buf):
        self._field = int(buf)
        LOG.append(('set_accel_field', int(buf)))

    @staticmethod
    def thermal_params(omega_t, t_ref, b, periodic):
        return (float(omega_t), float(t_ref), tuple(b), tuple(bool(p) for p in periodic))

    def thermal_init(self, module, params, gpu_map, gpu_t, gpu_v, g0, stream=None):
        LOG.append(('thermal_init', params, int(gpu_map), int(gpu_t), tuple(gpu_v), int(g0), stream))

    def thermal_step(self, module, params, gpu_map, g_src, g_dst, gpu_v, gpu_wall_t, gpu_t, stream=None):
        LOG.append(('thermal_step', params, int(gpu_map), int(g_src), int(g_dst), tuple(gpu_v), int(gpu_wall_t), int(gpu_t), stream))
        dim, dtype, nodes = self._shape(module)
        n = (2 * dim + 1) * nodes
        self._view(g_dst, dtype, n)[...] = self._view(g_src, dtype, n) + dtype(STEP)
        self._view(self._field, dtype, dim * nodes)[...] += dtype(STEP)

    def run_kernel(self, k, grid_size=None, stream=None):
        options = k.args[-1] if k.name == 'CollideAndPropagate' else None
        LOG.append(('run', k.name, options, stream))
        return super(ThermalRecordingBackend, self).run_kernel(k, grid_size, stream)


backend = ThermalRecordingBackend
