"""The CPU test backend (tests/_oracle_backend.py) with the acceleration-field call of backend_hip.HIPBackend, recording
what the runner does with it: LOG holds ('build', accel_field), ('set_accel_field', module, address, host copy of the
field), ('get_kernel', name) and ('run', name) in call order.  The oracle behind it knows no field: the numbers of such a
run mean nothing, the call sequence is what tests/test_accf_host.py reads.  Selected with backends='tests._accf_backend'.
Test-only."""
import ctypes

import numpy as np

from tests._oracle_backend import OracleBackend

LOG = []


class AccfRecordingBackend(OracleBackend):
    name = 'oracle_accf_test'

    @classmethod
    def add_options(cls, group):
        group.add_argument('--nohip_accel_field', dest='hip_accel_field', action='store_false', default=True)
        return OracleBackend.add_options(group)

    def build(self, source):
        LOG.append(('build', int(source.accel_field)))
        return super(AccfRecordingBackend, self).build(source)

    def set_accel_field(self, module, buf):
        d = module.desc
        dim = 2 if d.lattice == 0 else 3
        dtype = np.float32 if d.precision == 4 else np.float64
        n = dim * d.arr_nz * d.arr_ny * d.arr_nx
        raw = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(int(buf))
        field = np.frombuffer(raw, dtype=dtype, count=n).reshape(dim, d.arr_nz, d.arr_ny, d.arr_nx).copy()
        LOG.append(('set_accel_field', module, int(buf), field))

    def get_kernel(self, prog, name, *args, **kw):
        LOG.append(('get_kernel', name))
        return super(AccfRecordingBackend, self).get_kernel(prog, name, *args, **kw)

    def run_kernel(self, k, grid_size=None, stream=None):
        LOG.append(('run', k.name))
        return super(AccfRecordingBackend, self).run_kernel(k, grid_size, stream)


backend = AccfRecordingBackend
