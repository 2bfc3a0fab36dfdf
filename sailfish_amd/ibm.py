"""Immersed boundary markers on the device: the buffers of a set of markers and the three launches around a time step
(C ABI slf_ibm_*, csrc/slf_ibm.hip).  Used by subdomain_runner.IBMSubdomainRunner and, on a bare
box.BoxSim, by the tests.

A step of a simulation with markers is

    front():  slf_ibm_spread, slf_ibm_gather              (the spring forces become the module's acceleration field)
    the module's CollideAndPropagate with macroscopic output (the unchanged ACCF sweep: v is stored at every wet node)
    back():   slf_ibm_clear_and_advect                    (field and accumulator back to zero; x_p += interpolated v)

all on one stream.  The field buffer is the one handed to slf_module_set_accel_field; it must be zero before the first
front() and is zero again after every back()."""
import numpy as np


class Markers(object):
    def __init__(self, backend, module, dtype, dim, origin, position, ref_position, stiffness):
        """position, ref_position: [n, dim] global lattice coordinates; stiffness: [n]; origin: the global coordinates of
        the subdomain's first real node.  Allocates and uploads positions, reference positions and stiffness ([dim, n],
        [dim, n], [n] in `dtype`), the zeroed int64 accumulator and the per-marker `outside` words."""
        if not getattr(backend, 'supports_ibm', False):
            raise NotImplementedError('immersed boundary markers: backend %s has no slf_ibm_* calls' % getattr(backend, 'name', '?'))
        self.backend, self.module, self.dim = backend, module, dim
        self.origin = [int(x) for x in origin]
        pos = np.asarray(position, dtype=np.float64).reshape(-1, dim)
        ref = np.asarray(ref_position, dtype=np.float64).reshape(-1, dim)
        self.n = pos.shape[0]
        assert self.n > 0 and ref.shape == pos.shape
        self.position = np.ascontiguousarray(pos.T, dtype=dtype)            # [dim, n]: the host mirror
        self.ref_position = np.ascontiguousarray(ref.T, dtype=dtype)
        self.stiffness = np.ascontiguousarray(np.asarray(stiffness, dtype=np.float64).reshape(self.n), dtype=dtype)
        self.outside = np.zeros(self.n, dtype=np.uint32)
        b = backend
        self.gpu_position = b.alloc_buf(like=self.position)
        self.gpu_ref_position = b.alloc_buf(like=self.ref_position)
        self.gpu_stiffness = b.alloc_buf(like=self.stiffness)
        self.gpu_outside = b.alloc_buf(like=self.outside)
        self.acc_bytes = b.ibm_accumulator_bytes(module)
        self.acc = np.zeros(self.acc_bytes // 8, dtype=np.int64)
        self.gpu_acc = b.alloc_buf(like=self.acc)

    def front(self, stream):
        b = self.backend
        b.ibm_spread(self.module, self.n, self.origin, self.gpu_position, self.gpu_ref_position, self.gpu_stiffness,
                     self.gpu_acc, stream)
        b.ibm_gather(self.module, self.n, self.origin, self.gpu_position, self.gpu_acc, stream)

    def back(self, gpu_map, gpu_v, stream):
        self.backend.ibm_clear_and_advect(self.module, self.n, self.origin, self.gpu_position, self.gpu_acc, gpu_map, gpu_v,
                                          self.gpu_outside, stream)

    def positions(self, stream=None):
        """[n, dim] in the run's precision, copied back (waits for `stream`)."""
        if stream is not None:
            stream.synchronize()
        self.backend.from_buf(self.gpu_position)
        return np.array(self.position.T)

    def set_positions(self, position):
        self.position[...] = np.asarray(position).reshape(self.n, self.dim).T
        self.backend.to_buf(self.gpu_position)

    def outside_count(self, stream=None):
        """Markers the last back() held in place because their stencil leaves the subdomain's real nodes."""
        if stream is not None:
            stream.synchronize()
        self.backend.from_buf(self.gpu_outside)
        return int(self.outside.sum())

    def release(self):
        for addr in (self.gpu_position, self.gpu_ref_position, self.gpu_stiffness, self.gpu_outside, self.gpu_acc):
            self.backend.free_buf(addr)
