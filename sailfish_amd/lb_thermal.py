"""Thermal flows: a single fluid with a temperature field that it advects and that pushes back on it through buoyancy
(Boussinesq).  No counterpart in the reference; DESIGN.md §9j."""
import numpy as np

from sailfish_amd import subdomain_runner, thermal
from sailfish_amd.lb_base import LBForcedSim, ScalarField
from sailfish_amd.lb_single import LBFluidSim


class LBThermalFluidSim(LBFluidSim, LBForcedSim):
    """Single-phase simulation with a temperature lattice beside the sweep: D2Q5 with D2Q9, D3Q7 with D3Q19,
    BGK with tau_T = 1/2 + k --thermal_diffusivity (k = 3 / 4), always two-copy.  After every sweep one launch advances the
    temperature with the velocity the sweep has just stored and writes the buoyancy b (T - T_ref) into the module's
    acceleration field, which the next sweep reads (ThermalSubdomainRunner; csrc/slf_thermal.hip): the buoyancy lags the
    temperature by one step.  The module is an ordinary accel_field module, so what check_accel_field refuses is refused here
    too.  Uniform body forces (constant or time-dependent) add to the field as for any such module; a position-dependent body
    force would own the same buffer and is refused.

    Subdomains set `sim.T` (the initial temperature) and `sim.wall_temperature` in initial_conditions().  A node that is not
    wet -- a wall of any kind, an unused node behind a half-way wall -- with a finite wall_temperature holds that temperature
    at the mid-point of every link to a wet node; with NaN (the default) it is adiabatic.  A wet node with a finite
    wall_temperature (an inlet) is held at it -- in a subdomain with a node map; one whose every node is plain fluid runs the
    kernels that never read the node's own entry, so a finite entry there is refused (ValueError), not ignored.  Faces of
    the subdomain that are neither periodic nor walled are adiabatic."""
    subdomain_runner = subdomain_runner.ThermalSubdomainRunner
    has_accel_field = True

    def __init__(self, config):
        super(LBThermalFluidSim, self).__init__(config)
        self.buoyancy = [0.0] * self.grid.dim
        self.t_ref = 0.0
        self.thermal_g = None            # the current source copy of the temperature populations (checkpoints)
        self.thermal_field = None        # the acceleration field the next sweep reads (checkpoints)

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--thermal_diffusivity', type=float, default=1.0 / 6.0,
                           help='thermal diffusivity kappa > 0 (lattice units); tau_T = 1/2 + 3 kappa in 2-D, 1/2 + 4 kappa in 3-D')

    @classmethod
    def fields(cls):
        # wall_temperature is an input, NaN wherever nothing is imposed: not an output field
        return LBFluidSim.fields() + [ScalarField('T'), ScalarField('wall_temperature', init=np.nan, output=False)]

    @property
    def thermal_diffusivity(self):
        kappa = float(getattr(self.config, 'thermal_diffusivity', 1.0 / 6.0))
        if not kappa > 0.0:
            raise ValueError('--thermal_diffusivity must be > 0 (got %r)' % kappa)
        return kappa

    @property
    def tau_T(self):
        return thermal.tau_of(self.thermal_diffusivity, self.grid.dim)

    def set_buoyancy(self, vector, t_ref=0.0):
        """The buoyancy acceleration of a node is vector * (T - t_ref): vector = thermal expansion coefficient x gravity,
        pointing AGAINST gravity (hot fluid rises along it).  Call it from the constructor, like add_body_force."""
        if len(vector) != self.grid.dim:
            raise ValueError('the buoyancy of a %d-D simulation has %d components (got %d)'
                             % (self.grid.dim, self.grid.dim, len(vector)))
        self.buoyancy = [float(x) for x in vector]
        self.t_ref = float(t_ref)

    def add_body_force(self, force, grid=0, accel=True):
        from sailfish_amd import node_type as nt
        if isinstance(force, nt.DynamicValue) and force.space_dependent():
            raise NotImplementedError('LBThermalFluidSim: a body force that depends on position together with the buoyancy '
                                      'is not supported -- both would own the acceleration field (uniform forces, constant '
                                      'or time-dependent, are fine)')
        super(LBThermalFluidSim, self).add_body_force(force, grid, accel)

    def fill_module_desc(self, kw):
        super(LBThermalFluidSim, self).fill_module_desc(kw)
        self.thermal_diffusivity                          # (refuses a diffusivity that is not positive, before anything is built)
        kw['accel_field'] = 1
        kw['has_force'] = 1

    def accel_field_at(self, coords):
        """The field starts from zero: the init launch fills it with the buoyancy of the initial temperature."""
        return np.zeros((self.grid.dim, len(coords[0])), dtype=np.float64)

    def get_state(self):
        state = super(LBThermalFluidSim, self).get_state()
        if self.thermal_g is not None:
            state['thermal_g'] = np.array(self.thermal_g)
            state['thermal_field'] = np.array(self.thermal_field)
        return state

    def set_state(self, state):
        super(LBThermalFluidSim, self).set_state(state)
        if state.get('thermal_g') is not None:
            self.thermal_g = np.array(state['thermal_g'])
            self.thermal_field = np.array(state['thermal_field'])
