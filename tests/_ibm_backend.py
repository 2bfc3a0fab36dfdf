"""The CPU test backend (tests/_oracle_backend.py) with the marker calls of backend_hip.HIPBackend, recording what the
runner does with them: LOG holds ('build', accel_field), ('set_accel_field', address, host copy of the field),
('ibm_spread' | 'ibm_gather' | 'ibm_clear_and_advect', n, origin, ...) and ('run', kernel name, options) in call order.
The oracle behind it knows neither field nor markers, so the numbers of the fluid mean nothing; to make the positions
something a checkpoint can lose, ibm_clear_and_advect moves every marker by STEP along every axis (exact in both formats).
Selected with backends='tests._ibm_backend'.  Test-only."""
import ctypes

import numpy as np

from tests._oracle_backend import OracleBackend

LOG = []
STEP = 0.125


class IbmRecordingBackend(OracleBackend):
    name = 'oracle_ibm_test'
    supports_ibm = True

    @classmethod
    def add_options(cls, group):
        group.add_argument('--nohip_accel_field', dest='hip_accel_field', action='store_false', default=True)
        return OracleBackend.add_options(group)

    @staticmethod
    def _shape(module):
        d = module.desc
        dim = 2 if d.lattice == 0 else 3
        return dim, np.float32 if d.precision == 4 else np.float64, d.arr_nz * d.arr_ny * d.arr_nx

    def build(self, source):
        LOG.append(('build', int(source.accel_field)))
        return super(IbmRecordingBackend, self).build(source)

    def set_accel_field(self, module, buf):
        dim, dtype, nodes = self._shape(module)
        raw = (ctypes.c_char * (dim * nodes * np.dtype(dtype).itemsize)).from_address(int(buf))
        LOG.append(('set_accel_field', int(buf), np.frombuffer(raw, dtype=dtype, count=dim * nodes).copy()))

    def ibm_accumulator_bytes(self, module):
        dim, _, nodes = self._shape(module)
        return dim * nodes * 8

    def ibm_spread(self, module, n, origin, pos, ref, stiffness, acc, stream=None):
        LOG.append(('ibm_spread', int(n), tuple(origin), int(pos), int(ref), int(stiffness), int(acc), stream))

    def ibm_gather(self, module, n, origin, pos, acc, stream=None):
        LOG.append(('ibm_gather', int(n), tuple(origin), int(pos), int(acc), stream))

    def ibm_clear_and_advect(self, module, n, origin, pos, acc, gpu_map, gpu_v, outside, stream=None):
        LOG.append(('ibm_clear_and_advect', int(n), tuple(origin), int(pos), int(acc), int(gpu_map), tuple(gpu_v), int(outside),
                    stream))
        dim, dtype, _ = self._shape(module)
        raw = (ctypes.c_char * (dim * n * np.dtype(dtype).itemsize)).from_address(int(pos))
        np.frombuffer(raw, dtype=dtype, count=dim * n)[...] += dtype(STEP)

    def run_kernel(self, k, grid_size=None, stream=None):
        options = k.args[-1] if k.name == 'CollideAndPropagate' else None
        LOG.append(('run', k.name, options, stream))
        return super(IbmRecordingBackend, self).run_kernel(k, grid_size, stream)


backend = IbmRecordingBackend
