"""Binary-fluid models (reference sailfish/lb_binary.py): the Shan-Chen mixture and the free-energy model."""
import os
from collections import defaultdict, namedtuple

import numpy as np

from sailfish_amd import hipabi, serves, subdomain_runner, sym
from sailfish_amd.lb_base import LBForcedSim, LBSim, ScalarField, VectorField

MacroKernels = namedtuple('MacroKernels', 'distributions macro')

SHAN_CHEN_POTENTIALS = {'linear': 0, 'classic': 1}


class LBBinaryFluidBase(LBSim):
    """Two lattices (rho on lattice 0, the order parameter / second density phi on lattice 1), a shared
    velocity field and nearest-neighbour interactions (reference lb_binary.py:14-137)."""
    subdomain_runner = subdomain_runner.NNSubdomainRunner
    nonlocality = 1

    def __init__(self, config):
        super(LBBinaryFluidBase, self).__init__(config)
        self.grids.append(self.grid)

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--tau_phi', type=float, default=1.0, help='relaxation time for the phase field')

    def get_pbc_kernels(self, runner):
        """(distributions, macro) : copy -> axis -> kernels (reference lb_binary.py:40-105)."""
        dist_kernels = defaultdict(lambda: defaultdict(list))
        macro_kernels = defaultdict(lambda: defaultdict(list))
        if runner.indirect:      # periodic axes are wrapped inside the kernels; no ghost-layer kernels exist
            return MacroKernels(macro=macro_kernels, distributions=dist_kernels)
        d1a, d1b = runner.gpu_dist(0, 0), runner.gpu_dist(0, 1)
        d2a, d2b = runner.gpu_dist(1, 0), runner.gpu_dist(1, 1)
        nn_fields = [fp.buffer for fp in self._scalar_fields if fp.abstract.need_nn]
        for i in range(0, self.dim):
            dist_kernels[0][i] = [runner.get_kernel('ApplyPeriodicBoundaryConditions', [d1a, np.uint32(i)], 'Pi'),
                                  runner.get_kernel('ApplyPeriodicBoundaryConditions', [d2a, np.uint32(i)], 'Pi')]
        if self.config.access_pattern == 'AB':
            g1, g2, kernel = d1b, d2b, 'ApplyPeriodicBoundaryConditions'
        else:
            g1, g2, kernel = d1a, d2a, 'ApplyPeriodicBoundaryConditionsWithSwap'
        for i in range(0, self.dim):
            dist_kernels[1][i] = [runner.get_kernel(kernel, [g1, np.uint32(i)], 'Pi'),
                                  runner.get_kernel(kernel, [g2, np.uint32(i)], 'Pi')]
            for copy in (0, 1):
                macro_kernels[copy][i] = [runner.get_kernel('ApplyMacroPeriodicBoundaryConditions',
                                                            [runner.gpu_field(f), np.uint32(i)], 'Pi')
                                          for f in nn_fields]
        return MacroKernels(macro=macro_kernels, distributions=dist_kernels)

    def initial_conditions(self, runner):
        gpu_rho = runner.gpu_field(self.rho)
        gpu_phi = runner.gpu_field(self.phi)
        gpu_v = runner.gpu_field(self.v)
        gpu_map = runner.gpu_geo_map()
        args1 = [gpu_map, runner.gpu_dist(0, 0), runner.gpu_dist(1, 0)] + gpu_v + [gpu_rho, gpu_phi]
        runner.exec_kernel('SetInitialConditions', *runner.add_indirect_args(args1, 'P' * len(args1)))
        if self.config.access_pattern == 'AB':
            args2 = [gpu_map, runner.gpu_dist(0, 1), runner.gpu_dist(1, 1)] + gpu_v + [gpu_rho, gpu_phi]
            runner.exec_kernel('SetInitialConditions', *runner.add_indirect_args(args2, 'P' * len(args2)))

    def fill_module_desc(self, kw):
        super(LBBinaryFluidBase, self).fill_module_desc(kw)
        kw['tau_phi'] = self.config.tau_phi
        kw['model'] = hipabi.SLF_BGK


class LBBinaryFluidFreeEnergy(LBBinaryFluidBase):
    """Binary fluid mixture using the free-energy model (reference lb_binary.py:139-372), BGK: lattice 0 carries the
    density, lattice 1 the order parameter phi; surface tension sqrt(8 kappa A / 9), interface width sqrt(2 kappa / A)
    lattice units, viscosities through tau_a / tau_b, wetting full-way bounce-back walls (csrc/slf_fe.hip).  What the
    reference's model has beyond that -- the MRT collision, body forces, half-way wetting walls, other boundary
    conditions, indirect addressing -- is refused when the simulation is set up, by name."""

    # SetInitialConditions forms the Laplacian and the gradient of the host's phi: its ghost layer has to be filled first
    # (NNSubdomainRunner._gpu_initial_conditions)
    initial_conditions_need_nn = True

    @classmethod
    def fields(cls):
        return [ScalarField('rho'), ScalarField('phi', need_nn=True), VectorField('v'), ScalarField('phi_laplacian')]

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--bc_wall_grad_phase', type=float, default=0.0,
                           help='gradient of the phase field at the wall; this determines the wetting properties')
        group.add_argument('--bc_wall_grad_order', type=int, default=2, choices=[1, 2],
                           help='order of the gradient stencil used for the wetting boundary condition at the walls; '
                                'valid values are 1 and 2')
        group.add_argument('--Gamma', type=float, default=0.5, help='Gamma parameter')
        group.add_argument('--kappa', type=float, default=0.5, help='kappa parameter')
        group.add_argument('--A', type=float, default=0.5, help='A parameter')
        group.add_argument('--tau_a', type=float, default=1.0, help='relaxation time for the A component')
        group.add_argument('--tau_b', type=float, default=1.0, help='relaxation time for the B component')
        group.add_argument('--model', type=str, choices=['bgk', 'mrt'], default='bgk',
                           help='LB model to use (mrt: not implemented by the HIP backend)')

    def constants(self):
        c = self.config
        return {'Gamma': c.Gamma, 'A': c.A, 'kappa': c.kappa, 'tau_a': c.tau_a, 'tau_b': c.tau_b}

    def add_body_force(self, force, grid=0, accel=True):
        raise NotImplementedError('free-energy model: body forces (the reference\'s free_energy_external_force) are not '
                                  'implemented by the HIP backend')

    def use_force_for_equilibrium(self, force_grid, target_grid):
        raise NotImplementedError('free-energy model: use_force_for_equilibrium needs body forces '
                                  '(free_energy_external_force), which the HIP backend does not implement')

    def fill_module_desc(self, kw):
        super(LBBinaryFluidFreeEnergy, self).fill_module_desc(kw)
        c = self.config
        serves.check(serves.config_fields(c, simtype=hipabi.SLF_SIM_FREE_ENERGY), ('regularized / subgrid', 'free energy'),
                     columns=serves.COLUMNS)
        if c.bc_wall_grad_order not in (1, 2):
            raise ValueError('--bc_wall_grad_order must be 1 or 2')
        kw.update(lattice=self.grid.slf_id, simtype=hipabi.SLF_SIM_FREE_ENERGY,
                  # the fluid lattice relaxes with tau0(phi); tau / visc are what the generic checks look at
                  tau=c.tau_a, visc=(2.0 * c.tau_a - 1.0) / 6.0, incompressible=0,
                  fe_Gamma=c.Gamma, fe_kappa=c.kappa, fe_A=c.A, fe_tau_a=c.tau_a, fe_tau_b=c.tau_b,
                  bc_wall_grad_phase=c.bc_wall_grad_phase, bc_wall_grad_order=c.bc_wall_grad_order)

    @classmethod
    def check_module_desc(cls, kw):
        super(LBBinaryFluidFreeEnergy, cls).check_module_desc(kw)
        serves.check(kw, ('free energy',), always=True)

    @staticmethod
    def zero_gradient_rims(spec, dim):
        """Per axis 0 / 1 / 2: where the Laplacian and the gradient of phi are zero -- the reference's
        zero_gradient_at_boundaries (mako_utils.mako:168-197) with its `%if ... %elif` shape: on an axis that is neither
        locally periodic nor connected on its LOW face only the low rim layer (1); the high rim (2) is looked at only when
        the low face is connected."""
        faces = ((spec.X_LOW, spec.X_HIGH), (spec.Y_LOW, spec.Y_HIGH)) + (((spec.Z_LOW, spec.Z_HIGH),) if dim == 3 else ())
        rims = []
        for axis, (low, high) in enumerate(faces):
            periodic = bool(spec._periodicity[axis])
            if not periodic and not spec.has_face_conn(low):
                rims.append(1)
            elif not periodic and not spec.has_face_conn(high):
                rims.append(2)
            else:
                rims.append(0)
        return rims + [0] * (3 - dim)

    def fill_subdomain_desc(self, runner, kw):
        """What of the descriptor depends on the subdomain: the zero-gradient rims; and the check of the wetting walls."""
        kw['fe_zero_grad_rim'] = self.zero_gradient_rims(runner._spec, self.dim)
        self._check_wetting_walls(runner)

    def _check_wetting_walls(self, runner):
        """A full-way wall takes phi of the node bc_wall_grad_order nodes along its normal, formed from that node's
        populations (FreeEnergyPrepareMacroFields): it has to be a real node of this subdomain -- the ghost layer never
        holds a node's whole set of populations."""
        from sailfish_amd import node_type as nt
        sub, spec = runner._subdomain, runner._spec
        pos = np.argwhere(sub.visualization_map() == nt.NTFullBBWall.id)          # real nodes, numpy axis order
        if not len(pos):
            return
        order = int(self.config.bc_wall_grad_order)
        codes = sub._orientation[tuple(pos.T)].astype(np.int64)
        normal = np.array([list(reversed([int(c) for c in self.grid.dir_to_vec(int(code))])) if code else [0] * self.dim
                           for code in codes])
        helper = pos + order * normal
        shape = np.array(sub.lat_shape)
        for axis, wrapped in enumerate(reversed(runner._fused)):                  # axes the kernels wrap themselves
            if wrapped:
                helper[:, axis] %= shape[axis]
        outside = np.any((helper < 0) | (helper >= shape), axis=1)
        if outside.any():
            first = pos[np.nonzero(outside)[0][0]]
            where = tuple(int(c) + int(o) for c, o in zip(reversed(first), spec.location))
            raise ValueError('free-energy model: the wetting condition of the NTFullBBWall node %s reads the node %d nodes '
                             'along its normal, which lies outside subdomain %d (%d such wall nodes); move the seam, or use '
                             '--bc_wall_grad_order=1' % (where, order, spec.id, int(outside.sum())))

    def initial_conditions(self, runner):
        gpu_rho = runner.gpu_field(self.rho)
        gpu_phi = runner.gpu_field(self.phi)
        gpu_v = runner.gpu_field(self.v)
        gpu_map = runner.gpu_geo_map()
        copies = (0, 1) if self.config.access_pattern == 'AB' else (0,)
        for copy in copies:
            args = [gpu_map, runner.gpu_dist(0, copy), runner.gpu_dist(1, copy)] + gpu_v + [gpu_rho, gpu_phi]
            runner.exec_kernel('SetInitialConditions', args, 'P' * len(args))

    def get_compute_kernels(self, runner, full_output, bulk):
        """[(macro kernel, [fluid kernel, order-parameter kernel])] for the primary (A->B) and the secondary (B->A) half
        step, with the reference's argument lists (lb_binary.py:270-372).  The two sweeps run in this order: the second
        reads the velocity and the Laplacian the first stored."""
        gpu_rho = runner.gpu_field(self.rho)
        gpu_phi = runner.gpu_field(self.phi)
        gpu_lap = runner.gpu_field(self.phi_laplacian)
        gpu_v = runner.gpu_field(self.v)
        gpu_map = runner.gpu_geo_map()
        d1a, d1b = runner.gpu_dist(0, 0), runner.gpu_dist(0, 1)
        d2a, d2b = runner.gpu_dist(1, 0), runner.gpu_dist(1, 1)
        options = np.uint32((1 if full_output else 0) | (2 if bulk else 0))
        ni = self.config.needs_iteration_num

        def k(name, args):
            return runner.get_kernel(name, args + [options], 'P' * len(args) + 'i', needs_iteration=ni)

        def step(in1, out1, in2, out2):
            macro = k('FreeEnergyPrepareMacroFields', [gpu_map, in1, in2, gpu_rho, gpu_phi])
            fluid = k('FreeEnergyCollideAndPropagateFluid', [gpu_map, in1, out1, gpu_rho, gpu_phi] + gpu_v + [gpu_lap])
            order = k('FreeEnergyCollideAndPropagateOrderParam', [gpu_map, in2, out2, gpu_phi] + gpu_v + [gpu_lap])
            return macro, [fluid, order]

        primary = step(d1a, d1b, d2a, d2b)
        secondary = step(d1b, d1a, d2b, d2a) if self.config.access_pattern == 'AB' else primary
        return [primary, secondary]


class LBBinaryFluidShanChen(LBBinaryFluidBase, LBForcedSim):
    """Binary fluid mixture using the Shan-Chen model (reference lb_binary.py:375-517)."""

    @classmethod
    def fields(cls):
        return [ScalarField('rho', need_nn=True), ScalarField('phi', need_nn=True), VectorField('v')]

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--visc', type=float, default=1.0, help='numerical viscosity')
        group.add_argument('--G11', type=float, default=0.0,
                           help='Shan-Chen component 1 self-interaction strength constant')
        group.add_argument('--G12', type=float, default=0.0,
                           help='Shan-Chen component 1<->2 interaction strength constant')
        group.add_argument('--G22', type=float, default=0.0,
                           help='Shan-Chen component 2 self-interaction strength constant')
        group.add_argument('--sc_potential', type=str, choices=sorted(SHAN_CHEN_POTENTIALS), default='linear',
                           help='Shan-Chen pseudopotential function to use')

    def constants(self):
        c = self.config
        return {'G11': c.G11, 'G12': c.G12, 'G21': c.G12, 'G22': c.G22}

    def fill_module_desc(self, kw):
        super(LBBinaryFluidShanChen, self).fill_module_desc(kw)
        c = self.config
        kw.update(lattice=self.grid.slf_id, simtype=hipabi.SLF_SIM_SHAN_CHEN_BINARY,
                  tau=sym.relaxation_time(c.visc), visc=c.visc, mrt_rates=sym.mrt_rates(self.grid, c.visc),
                  incompressible=0, sc_G=[c.G11, c.G12, c.G12, c.G22],
                  sc_potential=SHAN_CHEN_POTENTIALS[c.sc_potential])

    def get_compute_kernels(self, runner, full_output, bulk):
        """[(macro kernel, [collide kernels])] for the primary (A->B) and the secondary (B->A) half step
        (reference lb_binary.py:418-517)."""
        gpu_rho = runner.gpu_field(self.rho)
        gpu_phi = runner.gpu_field(self.phi)
        gpu_v = runner.gpu_field(self.v)
        gpu_map = runner.gpu_geo_map()
        d1a, d1b = runner.gpu_dist(0, 0), runner.gpu_dist(0, 1)
        d2a, d2b = runner.gpu_dist(1, 0), runner.gpu_dist(1, 1)
        options = np.uint32((1 if full_output else 0) | (2 if bulk else 0))
        tail = [gpu_rho, gpu_phi] + gpu_v + [options]
        sig = 'P' * (4 + len(gpu_v) + 1) + 'i'
        ni = self.config.needs_iteration_num

        def k(name, a, b):
            # indirect addressing: the dense-node -> slot table leads the list (reference lb_binary.py:457-465)
            args, s = runner.add_indirect_args([gpu_map, a, b] + tail, sig)
            return runner.get_kernel(name, args, s, needs_iteration=ni)

        # backends that have it sweep both lattices in ONE pass (rho, phi and the pseudopotential stencil are read once;
        # C ABI kernels "ShanChenCollideAndPropagateFused[V]"), otherwise the reference's two kernels.  SLF_SC_FUSED:
        # 0 = the reference's kernels, 1 = fused sweep reading the velocity the pass in front stored, 2 (default) = fused
        # sweep forming the node's densities and velocity itself + "ShanChenPrepareDensities" in front of it, which stores
        # the velocity only in the full_output kernels (what the host reads after an output step)
        mode = os.environ.get('SLF_SC_FUSED', '2')
        fused = getattr(runner.backend, 'supports_fused_shan_chen', False) and getattr(self.config, 'hip_sc_fused', True) and \
            mode != '0' and not runner.indirect
        local_v = fused and mode != '1' and getattr(runner.backend, 'supports_fused_shan_chen_local_velocity', False)
        sweep_name = 'ShanChenCollideAndPropagateFusedV' if local_v else 'ShanChenCollideAndPropagateFused'
        macro_name = 'ShanChenPrepareDensities' if local_v else 'ShanChenPrepareMacroFields'

        def sweeps(in1, out1, in2, out2):
            if fused:
                return [runner.get_kernel(sweep_name, [gpu_map, in1, out1, in2, out2] + tail, 'PP' + sig, needs_iteration=ni)]
            return [k('ShanChenCollideAndPropagate0', in1, out1), k('ShanChenCollideAndPropagate1', in2, out2)]

        macro1 = k(macro_name, d1a, d2a)
        primary = sweeps(d1a, d1b, d2a, d2b)
        if self.config.access_pattern == 'AB':
            macro2 = k(macro_name, d1b, d2b)
            secondary = sweeps(d1b, d1a, d2b, d2a)
        else:
            macro2, secondary = macro1, primary
        return [(macro1, primary), (macro2, secondary)]
