"""The temperature lattice of a thermal flow on the device: its two copies and the launches around a time step (C ABI
slf_thermal_*, csrc/slf_thermal.hip).  Used by subdomain_runner.ThermalSubdomainRunner and, on a bare
box.BoxSim, by the tests.

A step of a thermal simulation is

    the module's CollideAndPropagate with macroscopic output (the unchanged ACCF sweep: v is stored at every wet node)
    back(it): slf_thermal_step                            (reads copy it & 1, writes the other; T and the field are rewritten)

on one stream, after one init() behind the flow's SetInitialConditions.  The field buffer is the one handed to
slf_module_set_accel_field: the sweep of step n reads the buoyancy of the temperature of step n - 1."""
import numpy as np

# directions per dimension, 1 / cs^2
Q = {2: 5, 3: 7}
K = {2: 3.0, 3: 4.0}


def tau_of(diffusivity, dim):
    """tau_T of a diffusivity: kappa = (tau_T - 1/2) / k with k = 3 on D2Q5 and 4 on D3Q7."""
    return 0.5 + K[dim] * float(diffusivity)


class ThermalLattice(object):
    def __init__(self, backend, module, dtype, dim, shape, periodic, diffusivity, t_ref, buoyancy, fill=0.0):
        """shape: the padded array shape of a field ((nz,) ny, nx as the module's arrays have it); periodic: the subdomain's
        locally periodic axes (x, y[, z]); buoyancy: dim components.  Allocates the two copies, filled with `fill` (a step
        never reads an entry no step or init() has written)."""
        if not getattr(backend, 'supports_thermal', False):
            raise NotImplementedError('thermal flows: backend %s has no slf_thermal_* calls' % getattr(backend, 'name', '?'))
        if not float(diffusivity) > 0.0:
            raise ValueError('thermal flows: the diffusivity must be > 0 (got %r)' % (diffusivity,))
        if len(buoyancy) != dim:
            raise ValueError('thermal flows: the buoyancy of a %d-D simulation has %d components' % (dim, dim))
        self.backend, self.module, self.dim, self.dtype = backend, module, dim, dtype
        self.tau = tau_of(diffusivity, dim)
        # omega_T: formed in double, rounded once to the run's precision
        self.omega = float(dtype(1.0 / self.tau))
        self.t_ref, self.buoyancy = float(t_ref), [float(x) for x in buoyancy]
        self.params = backend.thermal_params(self.omega, self.t_ref, self.buoyancy, [bool(p) for p in periodic])
        self.shape = (Q[dim],) + tuple(shape)
        self.host = [np.full(self.shape, fill, dtype=dtype) for _ in (0, 1)]        # host mirrors of the two copies
        # x = 1 of every row on a 128-byte line, like the fields the same lanes read and store
        kw = {'align_offset': backend.dist_align_offset(np.dtype(dtype).itemsize)} if hasattr(backend, 'dist_align_offset') else {}
        self.gpu_g = [backend.alloc_buf(like=h, **kw) for h in self.host]

    def init(self, gpu_map, gpu_t, gpu_v, stream):
        """Copy 0 = the equilibrium at (T, v); the field = the buoyancy of T.  Behind the flow's SetInitialConditions."""
        self.backend.thermal_init(self.module, self.params, gpu_map, gpu_t, gpu_v, self.gpu_g[0], stream)

    def back(self, it, gpu_map, gpu_v, gpu_wall_t, gpu_t, stream):
        """The thermal step of LB iteration `it`, behind its sweep."""
        src = it & 1
        self.backend.thermal_step(self.module, self.params, gpu_map, self.gpu_g[src], self.gpu_g[1 - src], gpu_v, gpu_wall_t,
                                  gpu_t, stream)

    def populations(self, copy, stream=None):
        """Copy `copy` as [Q] + shape, copied back (waits for `stream`)."""
        if stream is not None:
            stream.synchronize()
        self.backend.from_buf(self.gpu_g[copy])
        return np.array(self.host[copy])

    def set_populations(self, copy, values):
        self.host[copy][...] = np.asarray(values).reshape(self.shape)
        self.backend.to_buf(self.gpu_g[copy])

    def release(self):
        for addr in self.gpu_g:
            self.backend.free_buf(addr)
