"""Ternary-fluid models (reference sailfish/lb_ternary.py): the three-component Shan-Chen mixture."""
import os
from collections import defaultdict

import numpy as np

from sailfish_amd import hipabi, serves, subdomain_runner, sym
from sailfish_amd.lb_base import LBForcedSim, LBSim, ScalarField, VectorField
from sailfish_amd.lb_binary import MacroKernels, SHAN_CHEN_POTENTIALS


class LBTernaryFluidBase(LBSim):
    """Three lattices (rho on lattice 0, phi on lattice 1, theta on lattice 2), a shared velocity field and
    nearest-neighbour interactions (reference lb_ternary.py:14-152)."""
    subdomain_runner = subdomain_runner.NNSubdomainRunner
    nonlocality = 1

    def __init__(self, config):
        super(LBTernaryFluidBase, self).__init__(config)
        self.grids.append(self.grid)
        self.grids.append(self.grid)

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--tau_phi', type=float, default=1.0, help='relaxation time for the phase field 1 ')
        group.add_argument('--tau_theta', type=float, default=1.0, help='relaxation time for the phase field 2')

    @classmethod
    def visualization_fields(cls, dim):
        if dim == 2:
            return [ScalarField('v^2', expr=lambda f: np.square(f['vx']) + np.square(f['vy']))]
        return [ScalarField('v^2', expr=lambda f: np.square(f['vx']) + np.square(f['vy']) + np.square(f['vz']))]

    def _dists(self, runner, copy):
        return [runner.gpu_dist(k, copy) for k in range(3)]

    def get_pbc_kernels(self, runner):
        """(distributions, macro) : copy -> axis -> kernels (reference lb_ternary.py:44-116): the ghost-layer kernels run
        per lattice, the macro-field ones for the three density fields."""
        dist_kernels = defaultdict(lambda: defaultdict(list))
        macro_kernels = defaultdict(lambda: defaultdict(list))
        nn_fields = [fp.buffer for fp in self._scalar_fields if fp.abstract.need_nn]
        for i in range(0, self.dim):
            dist_kernels[0][i] = [runner.get_kernel('ApplyPeriodicBoundaryConditions', [d, np.uint32(i)], 'Pi')
                                  for d in self._dists(runner, 0)]
        if self.config.access_pattern == 'AB':
            dists, kernel = self._dists(runner, 1), 'ApplyPeriodicBoundaryConditions'
        else:
            dists, kernel = self._dists(runner, 0), 'ApplyPeriodicBoundaryConditionsWithSwap'
        for i in range(0, self.dim):
            dist_kernels[1][i] = [runner.get_kernel(kernel, [d, np.uint32(i)], 'Pi') for d in dists]
            for copy in (0, 1):
                macro_kernels[copy][i] = [runner.get_kernel('ApplyMacroPeriodicBoundaryConditions',
                                                            [runner.gpu_field(f), np.uint32(i)], 'Pi')
                                          for f in nn_fields]
        return MacroKernels(macro=macro_kernels, distributions=dist_kernels)

    def initial_conditions(self, runner):
        gpu_fields = [runner.gpu_field(self.rho), runner.gpu_field(self.phi), runner.gpu_field(self.theta)]
        gpu_v = runner.gpu_field(self.v)
        gpu_map = runner.gpu_geo_map()
        copies = (0, 1) if self.config.access_pattern == 'AB' else (0,)
        for copy in copies:
            args = [gpu_map] + self._dists(runner, copy) + gpu_v + gpu_fields
            runner.exec_kernel('SetInitialConditions', args, 'P' * len(args))

    def fill_module_desc(self, kw):
        super(LBTernaryFluidBase, self).fill_module_desc(kw)
        kw['tau_phi'] = self.config.tau_phi
        kw['tau_theta'] = self.config.tau_theta
        kw['model'] = hipabi.SLF_BGK


class LBTernaryFluidShanChen(LBTernaryFluidBase, LBForcedSim):
    """Ternary fluid mixture using the Shan-Chen model (reference lb_ternary.py:154-333; csrc/slf_sc3.hip).  What the
    kernels do not serve -- indirect addressing, collisions other than BGK, boundary conditions other than full-way
    bounce-back walls -- is refused when the simulation is set up, by name."""

    def __init__(self, config):
        super(LBTernaryFluidShanChen, self).__init__(config)
        self._force_couplings = {}
        for k in range(3):
            for j in range(3):
                self.add_force_coupling(k, j, 'G%d%d' % (k + 1, j + 1))

    def add_force_coupling(self, grid_a, grid_b, const_name):
        """A Shan-Chen coupling of lattice grid_a to the density of lattice grid_b through the constant const_name
        (reference lb_base.py:386-394); the kernels apply them in this order."""
        self._force_couplings[(grid_a, grid_b)] = const_name

    @classmethod
    def fields(cls):
        return [ScalarField('rho', need_nn=True), ScalarField('phi', need_nn=True), ScalarField('theta', need_nn=True),
                VectorField('v')]

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--visc', type=float, default=1.0, help='numerical viscosity')
        group.add_argument('--G11', type=float, default=0.0,
                           help='Shan-Chen component 1 self-interaction strength constant')
        group.add_argument('--G12', type=float, default=0.0,
                           help='Shan-Chen component 1<->2 interaction strength constant')
        group.add_argument('--G13', type=float, default=0.0,
                           help='Shan-Chen component 1<->3 interaction strength constant')
        group.add_argument('--G22', type=float, default=0.0,
                           help='Shan-Chen component 2 self-interaction strength constant')
        group.add_argument('--G23', type=float, default=0.0,
                           help='Shan-Chen component 2<->3 interaction strength constant')
        group.add_argument('--G33', type=float, default=0.0,
                           help='Shan-Chen component 3 self-interaction strength constant')
        group.add_argument('--sc_potential', type=str, choices=sorted(SHAN_CHEN_POTENTIALS), default='linear',
                           help='Shan-Chen pseudopotential function to use')

    def constants(self):
        c = self.config
        ret = super(LBTernaryFluidShanChen, self).constants()
        ret.update({'G11': c.G11, 'G12': c.G12, 'G13': c.G13,
                    'G21': c.G12, 'G22': c.G22, 'G23': c.G23,
                    'G31': c.G13, 'G32': c.G23, 'G33': c.G33})
        return ret

    def fill_module_desc(self, kw):
        super(LBTernaryFluidShanChen, self).fill_module_desc(kw)
        c = self.config
        serves.check(serves.config_fields(c, simtype=hipabi.SLF_SIM_SHAN_CHEN_TERNARY), ('regularized / subgrid', 'ternary Shan-Chen'),
                     columns=serves.COLUMNS)
        G = self.constants()
        kw.update(lattice=self.grid.slf_id, simtype=hipabi.SLF_SIM_SHAN_CHEN_TERNARY,
                  tau=sym.relaxation_time(c.visc), visc=c.visc, incompressible=0,
                  sc3_G=[G[self._force_couplings[(k, j)]] for k in range(3) for j in range(3)],
                  sc_potential=SHAN_CHEN_POTENTIALS[c.sc_potential])

    @classmethod
    def check_module_desc(cls, kw):
        super(LBTernaryFluidShanChen, cls).check_module_desc(kw)
        serves.check(kw, ('ternary Shan-Chen',), always=True)

    def get_compute_kernels(self, runner, full_output, bulk):
        """[(macro kernel, [collide kernels])] for the primary (A->B) and the secondary (B->A) half step, with the
        reference's kernel names and argument lists (lb_ternary.py:220-333)."""
        gpu_fields = [runner.gpu_field(self.rho), runner.gpu_field(self.phi), runner.gpu_field(self.theta)]
        gpu_v = runner.gpu_field(self.v)
        gpu_map = runner.gpu_geo_map()
        da, db = self._dists(runner, 0), self._dists(runner, 1)
        options = np.uint32((1 if full_output else 0) | (2 if bulk else 0))
        tail = gpu_fields + gpu_v + [options]
        ni = self.config.needs_iteration_num

        def k(name, dists):
            args = [gpu_map] + dists + tail
            return runner.get_kernel(name, args, 'P' * (len(args) - 1) + 'i', needs_iteration=ni)

        # backends that have it sweep the three lattices in ONE pass (the densities, the velocity and the pseudopotential
        # stencils are read once; C ABI kernel "ShanChenCollideAndPropagateFused" with three in / out pairs), otherwise the
        # reference's three kernels.  SLF_SC_FUSED=0: the reference's kernels.
        fused = getattr(runner.backend, 'supports_fused_shan_chen', False) and getattr(self.config, 'hip_sc_fused', True) and \
            os.environ.get('SLF_SC_FUSED', '2') != '0' and not runner.indirect

        def sweeps(src, dst):
            if fused:
                return [k('ShanChenCollideAndPropagateFused', [d for pair in zip(src, dst) for d in pair])]
            return [k('ShanChenCollideAndPropagate%d' % i, [src[i], dst[i]]) for i in range(3)]

        macro1 = k('ShanChenPrepareMacroFields', da)
        primary = sweeps(da, db)
        if self.config.access_pattern == 'AB':
            macro2 = k('ShanChenPrepareMacroFields', db)
            secondary = sweeps(db, da)
        else:
            macro2, secondary = macro1, primary
        return [(macro1, primary), (macro2, secondary)]
