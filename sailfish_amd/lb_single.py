"""Single-fluid LB simulation (reference sailfish/lb_single.py:14-240)."""
from collections import defaultdict

import numpy as np

from sailfish_amd import hipabi, serves, subdomain_runner, sym
from sailfish_amd.lb_base import KernelPair, LBForcedSim, LBSim, ScalarField, VectorField


class LBFluidSim(LBSim):
    """Simulates a single fluid."""
    subdomain_runner = subdomain_runner.SubdomainRunner
    alpha_output = False

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--visc', type=float, default=1.0, help='numerical viscosity')
        group.add_argument('--incompressible', action='store_true', default=False,
                           help='use the incompressible model of Luo and He')
        group.add_argument('--model', help='LB collision model to use', type=str, choices=['bgk', 'mrt', 'elbm'],
                           default='bgk')
        # the entropic collision (reference lb_single.py:31-50; templates/entropic.mako)
        group.add_argument('--entropic_equilibrium', action='store_true', default=False,
                           help='Use the equilibrium in product form instead of the standard LBGK equilibrium.')
        group.add_argument('--entropy_tolerance', type=float, default=0.0,
                           help='Entropy changes below this level will be treated as constant. If 0.0, a default value '
                                'depending on the precision of the simulation is used (1e-6 single, 1e-10 double).')
        group.add_argument('--alpha_tolerance', type=float, default=1e-10,
                           help='Alpha value tolerance used to end Newton-Raphson iterations.')
        # the two options of the reference's BGK relaxation preamble (lb_single.py:27-30, 38-42; relaxation_common.mako:166-237)
        group.add_argument('--regularized', action='store_true', default=False,
                           help='Apply the regularization procedure prior to the collision step.')
        group.add_argument('--subgrid', default='none', type=str, choices=['none', 'les-smagorinsky'],
                           help='subgrid model to use')
        group.add_argument('--smagorinsky_const', help='Smagorinsky constant', type=float, default=0.1)

    @classmethod
    def fields(cls):
        return [ScalarField('rho'), VectorField('v')]

    def fill_module_desc(self, kw):
        super(LBFluidSim, self).fill_module_desc(kw)
        cfg = self.config
        if not self.grid.model_supported(cfg.model):
            raise ValueError('model %s not supported on grid %s%s' % (
                cfg.model, self.grid.__name__, '' if hasattr(self.grid, 'mrt_matrix') else ' (the BGK collision only)'))
        kw.update(lattice=self.grid.slf_id,
                  model={'mrt': hipabi.SLF_MRT, 'elbm': hipabi.SLF_ELBM}.get(cfg.model, hipabi.SLF_BGK),
                  tau=sym.relaxation_time(cfg.visc), visc=cfg.visc,
                  mrt_rates=sym.mrt_rates(self.grid, cfg.visc),
                  incompressible=self.density_model(cfg))
        if getattr(cfg, 'entropic_equilibrium', False) and cfg.model != 'elbm':
            raise ValueError('--entropic_equilibrium is the equilibrium of the entropic collision: it needs --model=elbm')
        if cfg.model == 'elbm':
            kw.update(self.elbm_desc(self.grid, cfg.visc, cfg.precision, getattr(cfg, 'entropic_equilibrium', False),
                                     getattr(cfg, 'entropy_tolerance', 0.0), getattr(cfg, 'alpha_tolerance', 1e-10)))
        if getattr(cfg, 'regularized', False) or getattr(cfg, 'subgrid', 'none') != 'none':
            if cfg.model != 'bgk':
                # the reference's MRT relaxation never calls the preamble that implements them: it would ignore both silently
                raise ValueError('--regularized / --subgrid work with the BGK collision only')
            kw.update(regularized=int(bool(getattr(cfg, 'regularized', False))),
                      subgrid=hipabi.SLF_SUBGRID_LES_SMAGORINSKY if getattr(cfg, 'subgrid', 'none') == 'les-smagorinsky'
                      else hipabi.SLF_SUBGRID_NONE,
                      smagorinsky_const=float(getattr(cfg, 'smagorinsky_const', 0.1)))

    @staticmethod
    def elbm_tau0(grid, visc):
        """The relaxation time of the entropic collision, visc / cs^2 (reference lb_single.py:54-55); the populations
        relax by alpha beta with beta = 1 / (2 tau0 + 1)."""
        return visc / float(grid.cssq)

    @staticmethod
    def elbm_desc(grid, visc, precision, entropic_equilibrium=False, entropy_tolerance=0.0, alpha_tolerance=1e-10):
        """The slf_module_desc fields of an entropic module: the collision has one rate (no MRT rates), and an
        entropy_tolerance of 0 means the default of the precision (reference lb_single.py:63-67)."""
        if not entropy_tolerance > 0.0:
            entropy_tolerance = 1e-6 if precision == 'single' else 1e-10
        return dict(model=hipabi.SLF_ELBM, mrt_rates=[0.0] * grid.Q, entropic_equilibrium=int(bool(entropic_equilibrium)),
                    entropy_tolerance=float(entropy_tolerance), alpha_tolerance=float(alpha_tolerance))

    @staticmethod
    def density_model(cfg):
        """slf_module_desc::incompressible (SLF_DENSITY_*): the reference's three-way choice `incompressible` /
        `minimize_roundoff` / neither (sym.py:573-661, sym_equilibrium.py:100-118)."""
        if getattr(cfg, 'incompressible', False):
            return hipabi.SLF_DENSITY_INCOMPRESSIBLE
        if getattr(cfg, 'minimize_roundoff', False):
            if cfg.model != 'bgk':
                raise ValueError('--minimize_roundoff works with BGK-like models only (as in the reference)')
            return hipabi.SLF_DENSITY_ROUNDOFF
        return hipabi.SLF_DENSITY_COMPRESSIBLE

    ROUNDOFF_KINDS = tuple(k for k in range(32) if serves.BY_NAME['minimize_roundoff'].serves[-1] >> k & 1)

    @classmethod
    def check_module_desc(cls, kw):
        """Refuses, on the host and with a clear message, what the kernels of the chosen formulation do not cover
        (the library refuses the same at module creation)."""
        super(LBFluidSim, cls).check_module_desc(kw)
        serves.check(kw, ('minimize_roundoff',))
        if kw.get('entropic_equilibrium') and kw.get('model') != hipabi.SLF_ELBM:
            raise NotImplementedError('entropic_equilibrium needs model = elbm')
        if kw.get('model') == hipabi.SLF_ELBM:
            # what ELBM_relaxate (relaxation.mako:56-97) covers and this backend has fixtures for
            if any(float(x) != 0.0 for x in kw.get('mrt_rates', [])):
                raise NotImplementedError('--model=elbm: MRT relaxation rates are set; the entropic collision has one rate')
            serves.check(kw, ('elbm',))
            if kw.get('incompressible') == hipabi.SLF_DENSITY_INCOMPRESSIBLE and kw.get('entropic_equilibrium'):
                raise NotImplementedError('--model=elbm: --entropic_equilibrium (compressible product form) does not go with '
                                          '--incompressible')

    def initial_conditions(self, runner):
        """f = feq(rho, v) on every copy of the distributions (reference lb_single.py:72-94)."""
        gpu_rho = runner.gpu_field(self.rho)
        gpu_v = runner.gpu_field(self.v)
        gpu_map = runner.gpu_geo_map()
        args1 = [runner.gpu_dist(0, 0)] + gpu_v + [gpu_rho, gpu_map]
        runner.exec_kernel('SetInitialConditions', *runner.add_indirect_args(args1, 'P' * len(args1)))
        if self.config.access_pattern == 'AB':
            args2 = [runner.gpu_dist(0, 1)] + gpu_v + [gpu_rho, gpu_map]
            runner.exec_kernel('SetInitialConditions', *runner.add_indirect_args(args2, 'P' * len(args2)))

    def _compute_kernels_arguments(self, runner, full_output, bulk):
        gpu_rho = runner.gpu_field(self.rho)
        gpu_v = runner.gpu_field(self.v)
        gpu_dist1a = runner.gpu_dist(0, 0)
        gpu_dist1b = runner.gpu_dist(0, 1)
        gpu_map = runner.gpu_geo_map()
        assert len(gpu_v) == self.dim
        args1 = [gpu_map, gpu_dist1a, gpu_dist1b, gpu_rho] + gpu_v
        args2 = [gpu_map, gpu_dist1b, gpu_dist1a, gpu_rho] + gpu_v
        options = 0
        if full_output:
            options |= 1
        if bulk:
            options |= 2
        if getattr(self.config, 'check_invalid_results_gpu', False):
            options |= 4      # on-GPU invalid value check (slf_module_poll_invalid)
        args1.append(np.uint32(options))
        args2.append(np.uint32(options))
        signature = 'P' * (len(args1) - 1) + 'i'
        args1, sig1 = runner.add_indirect_args(args1, signature)
        args2, _ = runner.add_indirect_args(args2, signature)
        if self.alpha_output:
            # the alpha field of the entropic collision: the LAST argument (reference lb_single.py:129-133)
            args1.append(runner.gpu_field(self.alpha))
            args2.append(runner.gpu_field(self.alpha))
            sig1 += 'P'
        return sig1, args1, args2

    def get_compute_kernels(self, runner, full_output, bulk):
        signature, args1, args2 = self._compute_kernels_arguments(runner, full_output, bulk)
        cnp_primary = runner.get_kernel('CollideAndPropagate', args1, signature,
                                        needs_iteration=self.config.needs_iteration_num)
        if self.config.access_pattern == 'AB':
            cnp_secondary = runner.get_kernel('CollideAndPropagate', args2, signature,
                                              needs_iteration=self.config.needs_iteration_num)
            return KernelPair([cnp_primary], [cnp_secondary])
        return KernelPair([cnp_primary], [cnp_primary])

    def get_resident_kernels(self, runner, scratch, steps, tile, halo):
        """(forward, backward): `steps` time steps inside ONE launch for launch-bound 2-D subdomains (library kernel
        CollideAndPropagateResident, csrc/slf_resident.hip; no counterpart in the reference, which launches
        CollideAndPropagate once per step: subdomain_runner.py:960-974).  `forward` reads the distribution arrays and
        writes the scratch copies `scratch` = [copy A, copy B or 0], `backward` the other way round; the step the launch
        starts with is the kernel's iteration argument."""
        gpu_map = runner.gpu_geo_map()
        ab = self.config.access_pattern == 'AB'
        a, b = runner.gpu_dist(0, 0), (runner.gpu_dist(0, 1) if ab else 0)
        options = 4 if getattr(self.config, 'check_invalid_results_gpu', False) else 0
        ints = [np.uint32(options), np.uint32(steps), np.uint32(tile[0]), np.uint32(tile[1]), np.uint32(halo)]
        sig = 'PPPPPiiiii'
        fwd = runner.get_kernel('CollideAndPropagateResident', [gpu_map, a, b, scratch[0], scratch[1]] + ints, sig,
                                needs_iteration=True)
        bwd = runner.get_kernel('CollideAndPropagateResident', [gpu_map, scratch[0], scratch[1], a, b] + ints, sig,
                                needs_iteration=True)
        return fwd, bwd

    def get_pbc_kernels(self, runner):
        """grid copy (0 primary, 1 secondary) -> axis -> kernels (reference lb_single.py:153-185)."""
        if runner.indirect:      # periodic axes are wrapped inside the sweep; no ghost-layer kernels exist
            return defaultdict(lambda: defaultdict(list))
        gpu_dist1a = runner.gpu_dist(0, 0)
        gpu_dist1b = runner.gpu_dist(0, 1)
        kernels = defaultdict(lambda: defaultdict(list))
        for i in range(0, self.dim):
            kernels[0][i] = [runner.get_kernel('ApplyPeriodicBoundaryConditions',
                                               [gpu_dist1a, np.uint32(i)], 'Pi')]
        if self.config.access_pattern == 'AB':
            gpu_dist, kernel = gpu_dist1b, 'ApplyPeriodicBoundaryConditions'
        else:
            gpu_dist, kernel = gpu_dist1a, 'ApplyPeriodicBoundaryConditionsWithSwap'
        for i in range(0, self.dim):
            kernels[1][i] = [runner.get_kernel(kernel, [gpu_dist, np.uint32(i)], 'Pi')]
        return kernels


class LBEntropicFluidSim(LBFluidSim):
    """LBFluidSim with alpha field tracking (reference lb_single.py:202-218).

    The alpha field is 2.0 in areas where the fluid dynamics is fully resolved.  alpha < 2.0 means that the flow field is
    smoothened, while alpha > 2.0 indicates enhancement of flow perturbation.  The field is the last argument of
    CollideAndPropagate: the Newton iteration of a node starts from its previous alpha, and the alpha of every wet node
    is stored at every step.  It is written to the output like rho and travels with checkpoints (checkpoint_fields), so
    that a restored run resumes with the stored start values."""
    alpha_output = True
    checkpoint_fields = ('alpha',)

    @classmethod
    def modify_config(cls, config):
        config.model = 'elbm'

    @classmethod
    def fields(cls):
        return [ScalarField('rho'), VectorField('v'), ScalarField('alpha', init=2.0)]


class LBFreeSurface(LBFluidSim):
    """Shallow-water (free surface) lattice Boltzmann model (reference lb_single.py:221-239).

    `rho` is the water depth h and `v` the depth-averaged velocity; the pressure is gravity h^2 / 2 (--gravity), so small
    waves on a layer of depth h0 travel at sqrt(gravity h0).  D2Q9 and BGK, whatever --grid and --model say.  The moving
    populations relax towards the reference's equilibrium; the rest population relaxes towards h minus their sum, which
    conserves the water volume exactly -- the reference's own rest population does not (its equilibrium sums to
    h + 2 h v^2), and there is no switch back to it.  Walls are NTFullBBWall, NTHalfBBWall and NTSlip; the node types that
    carry a density or a velocity are refused.  The kernels read --gravity rounded to single precision, in both precisions
    (the module descriptor carries it as a float).  With LBForcedSim, body forces act as on any single fluid: a bed slope is
    the acceleration -gravity grad z_b, a function of position (add_body_force(DynamicValue(...)))."""

    @classmethod
    def modify_config(cls, config):
        # the reference overrides both silently; a collision model somebody asked for is refused by name instead (bgk is
        # the default of --model, so anything else was typed)
        model = getattr(config, 'model', 'bgk')
        if model != 'bgk':
            raise NotImplementedError('shallow water (LBFreeSurface): --model=%s is not served; the BGK collision only' % model)
        config.grid = 'D2Q9'
        config.model = 'bgk'

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--gravity', type=float, default=0.001, help='gravitational acceleration')

    def constants(self):
        ret = super(LBFreeSurface, self).constants()
        ret['gravity'] = self.config.gravity
        return ret

    def fill_module_desc(self, kw):
        super(LBFreeSurface, self).fill_module_desc(kw)
        kw.update(equilibrium=hipabi.SLF_EQ_SHALLOW_WATER, gravity=float(self.config.gravity))
        # what the command line alone decides is refused here, before the geometry is encoded (check_module_desc sees the
        # node types later); the addressing is not part of `kw` yet
        indirect = getattr(self.config, 'node_addressing', 'direct') == 'indirect'
        self.check_shallow_water(dict(kw, node_addressing=hipabi.SLF_ADDR_INDIRECT if indirect else hipabi.SLF_ADDR_DIRECT))

    # CollideAndPropagateResident implements the BGK polynomial and does not exist in a shallow-water module: the class
    # has no such kernels (SubdomainRunner._resident_setup asks with hasattr), so small boxes run one launch per step
    @property
    def get_resident_kernels(self):
        raise AttributeError('LBFreeSurface has no several-steps-per-launch kernels')


class LBSingleFluidShanChen(LBFluidSim, LBForcedSim):
    """Single-component Shan-Chen model (reference lb_single.py:242-347): every step computes the density
    field first (PrepareMacroFields), then collides with the pseudopotential force added by Guo forcing."""
    nonlocality = 1
    subdomain_runner = subdomain_runner.NNSubdomainRunner

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--G', type=float, default=1.0, help='Shan-Chen interaction strength constant')
        group.add_argument('--sc_potential', type=str, choices=['classic', 'linear'], default='linear',
                           help='Shan-Chen pseudopotential function to use')

    @classmethod
    def fields(cls):
        return [ScalarField('rho', need_nn=True), VectorField('v')]

    def constants(self):
        return {'SCG': self.config.G}

    def fill_module_desc(self, kw):
        super(LBSingleFluidShanChen, self).fill_module_desc(kw)
        if self.config.model != 'bgk':
            raise ValueError('the Shan-Chen model uses the BGK collision operator')
        kw.update(simtype=hipabi.SLF_SIM_SHAN_CHEN_SINGLE, sc_G=[self.config.G, 0.0, 0.0, 0.0],
                  sc_potential={'linear': 0, 'classic': 1}[self.config.sc_potential], tau_phi=kw['tau'])

    def get_pbc_kernels(self, runner):
        from sailfish_amd.lb_binary import MacroKernels
        dist_kernels = super(LBSingleFluidShanChen, self).get_pbc_kernels(runner)
        macro_kernels = defaultdict(lambda: defaultdict(list))
        for copy in (0, 1):
            for i in range(0, self.dim):
                macro_kernels[copy][i] = [runner.get_kernel('ApplyMacroPeriodicBoundaryConditions',
                                                            [runner.gpu_field(fp.buffer), np.uint32(i)], 'Pi')
                                          for fp in self._scalar_fields if fp.abstract.need_nn]
        return MacroKernels(macro=macro_kernels, distributions=dist_kernels)

    def get_compute_kernels(self, runner, full_output, bulk):
        gpu_rho = runner.gpu_field(self.rho)
        gpu_map = runner.gpu_geo_map()
        options = np.uint32((1 if full_output else 0) | (2 if bulk else 0))
        ni = self.config.needs_iteration_num
        macro_kernels = []
        for c in (0, 1):
            args, sig = runner.add_indirect_args([gpu_map, runner.gpu_dist(0, c), gpu_rho, options], 'PPPi')
            macro_kernels.append(runner.get_kernel('PrepareMacroFields', args, sig, needs_iteration=ni))
        sim_kernels = super(LBSingleFluidShanChen, self).get_compute_kernels(runner, full_output, bulk)
        return list(zip(macro_kernels, sim_kernels))


class Particle(object):
    """An immersed boundary marker (reference lb_single.py:406-411): a position in global lattice coordinates -- those of
    hx, hy, hz: a node sits at integer coordinates --, tied to ref_position (default: where it starts) by a spring of
    the given stiffness.  `mass` is kept for script compatibility; nothing reads it (nor does the reference)."""

    def __init__(self, position, mass=1.0, stiffness=1.0, ref_position=None):
        self.position = tuple(float(x) for x in position)
        self.mass = mass
        self.ref_position = self.position if ref_position is None else tuple(float(x) for x in ref_position)
        self.stiffness = float(stiffness)
        assert len(self.ref_position) == len(self.position)


class LBIBMFluidSim(LBFluidSim, LBForcedSim):
    """Single-phase simulation with immersed boundary markers (reference lb_single.py:350-404).  The markers'
    spring forces are spread into the module's acceleration field before every step and the markers move with the
    interpolated fluid velocity after it (IBMSubdomainRunner; csrc/slf_ibm.hip).  The module is an ordinary accel_field
    module, so what check_accel_field refuses is refused here too.  Uniform body forces (constant or time-dependent) add to
    the field as for any such module; a position-dependent body force would own the same buffer and is refused.
    `particle_positions` ([n, dim], the run's precision) is refreshed whenever the fields are copied to the host, and
    travels with checkpoints."""
    subdomain_runner = subdomain_runner.IBMSubdomainRunner
    has_accel_field = True

    def __init__(self, config):
        super(LBIBMFluidSim, self).__init__(config)
        self._particles = []
        self.particle_positions = None

    @classmethod
    def fields(cls):
        # `force`: the reference's per-node force field, kept so that scripts which name sim.force load; the kernels here read
        # the module's acceleration field instead, and this one stays zero
        return LBFluidSim.fields() + [VectorField('force')]

    @property
    def num_particles(self):
        return len(self._particles)

    def add_particle(self, particle):
        assert isinstance(particle, Particle)
        if len(particle.position) != self.grid.dim:
            raise ValueError('a particle of a %d-D simulation has %d coordinates' % (self.grid.dim, self.grid.dim))
        self._particles.append(particle)

    def add_body_force(self, force, grid=0, accel=True):
        from sailfish_amd import node_type as nt
        if isinstance(force, nt.DynamicValue) and force.space_dependent():
            raise NotImplementedError('LBIBMFluidSim: a body force that depends on position together with immersed boundary '
                                      'markers is not supported -- both would own the acceleration field (uniform forces, '
                                      'constant or time-dependent, are fine)')
        super(LBIBMFluidSim, self).add_body_force(force, grid, accel)

    def fill_module_desc(self, kw):
        super(LBIBMFluidSim, self).fill_module_desc(kw)
        kw['accel_field'] = 1
        kw['has_force'] = 1

    def accel_field_at(self, coords):
        """The field starts from zero: the markers fill it before every step."""
        return np.zeros((self.grid.dim, len(coords[0])), dtype=np.float64)

    def get_state(self):
        state = super(LBIBMFluidSim, self).get_state()
        if self.particle_positions is not None:
            state['particle_positions'] = np.array(self.particle_positions)
        return state

    def set_state(self, state):
        super(LBIBMFluidSim, self).set_state(state)
        if state.get('particle_positions') is not None:
            self.particle_positions = np.array(state['particle_positions'])
