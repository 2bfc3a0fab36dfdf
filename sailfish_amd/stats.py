"""Flow statistics formed on the device (reference sailfish/stats.py): global kinetic energy and enstrophy, and the
profiles of moments and correlations along one axis that characterise a turbulent flow.

Mix one of the classes into a simulation::

    class KidaSim(LBFluidSim, KineticEnergyEnstrophyMixIn):
        def after_step(self, runner):
            mod = self.iteration % 20
            if mod == 19:
                self.need_fields_flag = True          # the NEXT step stores rho and v
            elif mod == 0:
                ke, ens = self.compute_ke_enstropy(runner)

Stale fields.  The statistics read the density and velocity arrays of the device AS THEY ARE.  The sweeps store those
arrays only in steps that were asked for them (output, or `need_fields_flag` / `need_sync_flag` set during the step
before, as above and as in the reference); in between they keep the values of the last such step.  A simulation that
overrides `after_step` is stepped one step at a time (SubdomainRunner._steps_without_host returns 0 for it), so the
flag always takes effect in the following step.

What the fields hold at nodes that are not fluid: wet boundary-condition nodes their own density and velocity; dry
nodes (full-way bounce-back walls, slip walls) and unused nodes are never written by the sweeps and keep what the
initial conditions put there -- 0 unless the subdomain's initial_conditions() says otherwise (`sim.rho[:] = 1.0` sets
the walls' density to 1).  The energy and enstrophy sums leave out excluded nodes (unused, propagation-only) but, like
the reference, count dry wall nodes, and differentiate across whatever the neighbour holds; the profiles count every
real node and do not look at the node map at all (reference templates/reynolds_statistics.mako).

The kernels are sailfish_amd/csrc/slf_stats.hip behind the C ABI's slf_stats_* entry points.  3-D simulations only.
"""
import numpy as np

from sailfish_amd import hipabi
from sailfish_amd.lb_base import LBMixIn, ScalarField

#: the statistics of a profile in the order of the device buffer (include/sailfish_hip.h, slf_stats_profiles)
PROFILE_KEYS = tuple('%s_m%d' % (f, m) for f in ('ux', 'uy', 'uz', 'rho') for m in range(1, 5)) + \
    ('ux_uy', 'ux_uz', 'uy_uz', 'ux_rho', 'uy_rho', 'uz_rho')
assert len(PROFILE_KEYS) == hipabi.SLF_STATS_PROFILE_COUNT


def _require_3d(sim, what):
    if sim.dim != 3:
        raise NotImplementedError('%s needs a 3-D simulation: the statistics read vx, vy and vz (this one is %d-D)'
                                  % (what, sim.dim))


def _settle(runner):
    """The field stores of a step that split its sweep over two streams are complete (SubdomainRunner._fields_to_host)."""
    bs = getattr(runner, '_bnd_stream', None)
    if bs is not None and bs is not runner._calc_stream:
        bs.synchronize()


class FlowStatsMixIn(LBMixIn):
    """When mixed with an LBFluidSim-descendant class, provides easy access to various flow statistics."""


class KineticEnergyEnstrophyMixIn(FlowStatsMixIn):
    """Computes global kinetic energy and enstrophy densities.  See the module docstring for when the device fields are
    current."""

    @classmethod
    def fields(cls):
        return [ScalarField('v_sq', gpu_array=True, init=0.0),
                ScalarField('vort_sq', gpu_array=True, init=0.0)]

    def before_main_loop(self, runner):
        _require_3d(self, 'KineticEnergyEnstrophyMixIn')
        if getattr(self, '_ke_runner', None) is runner:
            return          # (the runner calls the hooks of mix-ins itself; a simulation may have called this one too)
        b = runner.backend
        self._ke_runner = runner
        self._ke_workspace = b.stats_workspace(runner.module, hipabi.SLF_STATS_KE_ENSTROPHY)
        self._ke_sums = b.alloc_async_host_buf((2,), np.float64)      # pinned: the read-back is 16 bytes and a latency
        self._ke_gpu_sums = b.alloc_buf(like=self._ke_sums)
        # a fluid-only module has no node the sums could leave out: the map is not read
        self._ke_map = 0 if int(runner._desc.fluid_only) else runner.gpu_geo_map()

    def compute_ke_enstropy(self, runner, store_fields=True):
        """Computes kinetic energy and enstrophy densities on the compute device.

        :param store_fields: also store the per-node values in the device arrays of `v_sq` and `vort_sq` (the
            reference always does); the returned numbers are the same bits either way
        :rvalue: kinetic energy, enstrophy (per node)
        """
        b = runner.backend
        _settle(runner)
        b.stats_ke_enstrophy(runner.module, self._ke_map, runner.gpu_field(self.v), self._ke_workspace, self._ke_gpu_sums,
                             runner.gpu_field(self.v_sq) if store_fields else 0,
                             runner.gpu_field(self.vort_sq) if store_fields else 0, runner._calc_stream)
        b.from_buf_async(self._ke_gpu_sums, runner._calc_stream)
        b.sync_stream(runner._calc_stream)
        div = 2.0 * runner._spec.num_nodes
        return float(self._ke_sums[0]) / div, float(self._ke_sums[1]) / div


class ReynoldsStatsMixIn(FlowStatsMixIn):
    """Computes statistics used to characterize turbulent flows:
    - first 4 moments of any quantity (velocity, density)
    - correlations between any 2 quantities
    as profiles along one axis, averaged over the two others.  See the module docstring for when the device fields are
    current and for what they hold at wall nodes.
    """

    #: Number of copies of the stats buffers to keep in GPU memory between host syncs.
    stat_buf_size = 1024

    stat_cnt = 0

    def prepare_reynolds_stats(self, runner, moments=True, correlations=True, axis='x'):
        """Allocates the device ring of `stat_buf_size` snapshots along `axis` ('x', 'y' or 'z').  One pass forms all 22
        statistics; `moments` / `correlations` are kept for the reference's signature."""
        _require_3d(self, 'ReynoldsStatsMixIn')
        if axis not in ('x', 'y', 'z'):
            raise ValueError("axis must be 'x', 'y' or 'z'")
        ax = 'xyz'.index(axis)
        size = runner._spec.size                 # this subdomain's own extents (nx, ny, nz)
        b = runner.backend
        self._reyn_axis = ax
        self._reyn_points = int(size[ax])
        self._reyn_moments = moments
        self._reyn_corr = correlations
        self._reyn_normalizer = int(np.prod(size, dtype=np.int64)) // int(size[ax])
        self._reyn_ring = np.zeros((len(PROFILE_KEYS), self.stat_buf_size, self._reyn_points), dtype=np.float64)
        self._reyn_bytes = self._reyn_ring.nbytes
        self._reyn_gpu_ring = b.alloc_buf(like=self._reyn_ring)
        self._reyn_workspace = b.stats_workspace(runner.module, hipabi.SLF_STATS_PROFILES_X + ax)
        self.stat_cnt = 0
        #: List of iterations at which measurements were taken.
        self.snapshot_iters = []
        self.config.logger.info('Size of Reynolds stats buffer: %d' % self._reyn_bytes)

    def collect_reynolds_stats(self, runner):
        """Collects Reynolds statistics: one snapshot into the device ring.  Returns None until the ring is full; then
        the dictionary of the 22 statistics, each [stat_buf_size, N] and divided by the number of nodes per position,
        plus 'iters', and starts over."""
        b = runner.backend
        n = self._reyn_points
        _settle(runner)
        b.stats_profiles(runner.module, self._reyn_axis, runner.gpu_field(self.v), runner.gpu_field(self.rho),
                         self._reyn_workspace, self._reyn_gpu_ring, self.stat_buf_size * n, self.stat_cnt * n,
                         runner._calc_stream)
        self.stat_cnt += 1
        self.snapshot_iters.append(self.iteration)
        if self.stat_cnt < self.stat_buf_size:
            return None
        self.stat_cnt = 0
        b.from_buf_async(self._reyn_gpu_ring, runner._calc_stream)
        b.sync_stream(runner._calc_stream)
        div = self._reyn_normalizer
        iters, self.snapshot_iters = self.snapshot_iters, []
        out = dict((key, self._reyn_ring[k] / div) for k, key in enumerate(PROFILE_KEYS))
        out['iters'] = iters
        return out
