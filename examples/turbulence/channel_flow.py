#!/usr/bin/env python
"""Turbulent flow between two parallel plates, driven by a body force (the flow of sailfish's
examples/turbulence/channel_flow.py; same option names: --H, --Re_tau, --wall, --external_perturbation).

The plates are normal to x, the flow runs along z and y is the spanwise direction; y and z are periodic and subdomains
are cut along z, so what neighbours exchange are whole planes.  The box is 2 H x 2 H x 6 H nodes (about the geometry of
Moser, Kim and Mansour) plus the wall layers.  --wall picks the no-slip wall: 'hbb' full-way bounce-back nodes, 'bbl'
half-way bounce-back on the links, 'tms' the Tamm-Mott-Smith wall (Chikatamarla and Karlin, Physica A 392 (2013) 1925).

The initial state is the log-law profile (linear in the viscous sublayer) with a divergence-free perturbation on top:
the curl of a smoothed random vector potential, or fields loaded from --external_perturbation.  After two flow-through
times, Reynolds statistics (sailfish.stats.ReynoldsStatsMixIn, profiles along x) are sampled every 20 steps and written
to <output>/reyn_stats/stats_<subdomain id>.<iteration>.npz whenever the device ring of snapshots is full.
--stats_after / --stats_snapshots change when the sampling starts and how many snapshots make a file."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # repo root (the `sailfish` alias)

import numpy as np
import scipy.ndimage

from sailfish.controller import LBSimulationController
from sailfish.geo import EqualSubdomainsGeometry3D
from sailfish.lb_base import LBForcedSim
from sailfish.lb_single import LBFluidSim
from sailfish.node_type import NTFullBBWall, NTHalfBBWall, NTWallTMS
from sailfish.stats import ReynoldsStatsMixIn
from sailfish.subdomain import Subdomain3D

KARMAN = 0.41
LOG_LAW_B = 5.5
SUBLAYER_EDGE = 11.44532166          # y+ at which u+ = y+ meets the log law
PAD = 40                             # extra nodes around the random field that make it periodic along y and z
SAMPLE_EVERY = 20


def log_law(y_plus):
    """u+ of the log law."""
    return np.log(y_plus) / KARMAN + LOG_LAW_B


class ChannelSubdomain(Subdomain3D):
    u0 = 0.05                        # centre-line velocity of the initial profile
    wall_bc = NTFullBBWall           # set from --wall (ChannelSim.modify_config)

    @classmethod
    def u_tau(cls, Re_tau):
        """Friction velocity: the log law reaches u0 at the centre line, which is y+ = Re_tau."""
        return cls.u0 / float(log_law(Re_tau))

    def boundary_conditions(self, hx, hy, hz):
        self.set_node((hx == 0) | (hx == self.gx - 1), self.wall_bc)

    def initial_conditions(self, sim, hx, hy, hz):
        sim.rho[:] = 1.0
        cfg = self.config
        H = cfg.H
        u_tau = self.u_tau(cfg.Re_tau)
        # distance from the nearer wall, which sits wall_bc.location node spacings off the outermost node layer
        from_centre = np.abs(hx - self.wall_bc.location - H)
        assert np.all((H - from_centre)[hx == 0] == -self.wall_bc.location)
        y_plus = (H - from_centre + 1) * u_tau / cfg.visc
        u = np.where(y_plus < SUBLAYER_EDGE, y_plus, log_law(np.maximum(y_plus, 1e-30))) * u_tau
        sim.vz[:] = u
        dv = self.perturbation(hx, hy, hz)
        assert all(np.isfinite(c).all() for c in dv)
        amplitude = 0.03 * u / self.u0      # the largest perturbation: 0.03 where the profile reaches u0
        sim.vx[:] += dv[0] * amplitude
        sim.vy[:] += dv[1] * amplitude
        sim.vz[:] += dv[2] * amplitude

    # -- the perturbation: one field over the whole channel, the same in every subdomain, of which each takes its own
    # part; it is scaled by its largest component over the WHOLE channel, so that the initial state does not depend on
    # how the channel is cut into subdomains
    def _own_part(self, field, hx, hy, hz):
        return field[hz.min():hz.max() + 1, hy.min():hy.max() + 1, hx.min():hx.max() + 1]

    def _smooth_gradients(self):
        """Gradients (d/dz, d/dy, d/dx) of one smoothed random scalar field that is continuous across the periodic faces."""
        half = PAD // 2
        noise = np.random.random((self.gz + PAD, self.gy + PAD, self.gx)).astype(np.float32) * 2.0 - 1.0
        noise[-half:, :, :] = noise[half:PAD, :, :]
        noise[:half, :, :] = noise[-PAD:-half, :, :]
        noise[:, -half:, :] = noise[:, half:PAD, :]
        noise[:, :half, :] = noise[:, -PAD:-half, :]
        smooth = scipy.ndimage.gaussian_filter(noise, 5 * self.config.H // 40)
        return [g[half:-half, half:-half, :] for g in np.gradient(smooth)]

    def perturbation(self, hx, hy, hz):
        """(dvx, dvy, dvz) on this subdomain's nodes, largest component over the channel 1: the curl of a random vector
        potential, or the fields of --external_perturbation."""
        ext = self.config.external_perturbation
        if ext:
            base = os.path.join(ext, 'rng_%d_%d_%d_' % (self.gx, self.gy, self.gz))
            dv = [np.load(base + 'dv%s.npz' % c)['data'] for c in 'xyz']
        else:
            np.random.seed(self.config.seed)
            # (d/dz, d/dy, d/dx) of the three components of the potential; the velocity is its curl
            (ax_z, ax_y, _), (ay_z, _, ay_x), (_, az_y, az_x) = [self._smooth_gradients() for _ in range(3)]
            dv = [az_y - ay_z, ax_z - az_x, ay_x - ax_y]
        scale = max(float(np.max(np.abs(c))) for c in dv)
        return [self._own_part(c, hx, hy, hz) / scale for c in dv]


class ChannelSim(LBFluidSim, LBForcedSim, ReynoldsStatsMixIn):
    subdomain = ChannelSubdomain
    walls = {'hbb': NTFullBBWall, 'bbl': NTHalfBBWall, 'tms': NTWallTMS}

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({
            'access_pattern': 'AA', 'grid': 'D3Q19', 'force_implementation': 'guo', 'model': 'bgk',
            'minimize_roundoff': True, 'precision': 'single', 'seed': 1341351351,
            'periodic_y': True, 'periodic_z': True, 'conn_axis': 'z',
            'check_invalid_results_gpu': False, 'block_size': 128,
            'max_iters': 3500000, 'every': 200000, 'perf_stats_every': 5000,
            'final_checkpoint': True, 'checkpoint_every': 500000,
            # the options of this script, for runs that are configured without its command line
            'H': 40, 'Re_tau': 180.0, 'wall': 'hbb', 'external_perturbation': '', 'stats_after': -1, 'stats_snapshots': 0,
        })

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--H', type=int, default=40, help='half the distance between the plates, in node spacings')
        group.add_argument('--Re_tau', type=float, default=180.0, help='friction Reynolds number u_tau H / visc the force and the viscosity are set for')
        group.add_argument('--wall', choices=('hbb', 'bbl', 'tms'), default='hbb', help='node type of the plates: full-way bounce-back, half-way bounce-back, Tamm-Mott-Smith')
        group.add_argument('--external_perturbation', type=str, default='',
                           help='directory of rng_<nx>_<ny>_<nz>_dv{x,y,z}.npz: the perturbation to use instead of the random one')
        group.add_argument('--stats_after', type=int, default=-1,
                           help='Iteration after which Reynolds statistics are sampled (default: two flow-through times).')
        group.add_argument('--stats_snapshots', type=int, default=0,
                           help='Snapshots per statistics file (default: the size of the device ring, 1024).')

    @classmethod
    def modify_config(cls, config):
        wall = cls.walls[config.wall]
        cls.subdomain.wall_bc = wall
        layers = 2 if wall.location == 0.5 else 0        # node layers the walls take beyond the 2 H of fluid
        config.lat_nx = 2 * config.H + layers            # wall-normal
        config.lat_ny = 2 * config.H                     # spanwise
        config.lat_nz = 6 * config.H                     # streamwise
        config.visc = cls.subdomain.u_tau(config.Re_tau) * config.H / config.Re_tau
        if not getattr(config, 'quiet', False):
            print('\n'.join(cls.describe(config)))

    @classmethod
    def t_char(cls, config):
        return config.H / cls.subdomain.u_tau(config.Re_tau)

    @classmethod
    def t_flow(cls, config):
        """Flow-through time at the friction velocity."""
        return cls.t_char(config) * (config.lat_nz / config.H)

    @classmethod
    def force(cls, config):
        """u_tau^2 / H: the wall shear stress of the target Re_tau balances it."""
        return config.Re_tau ** 2 * config.visc ** 2 / config.H ** 3

    @classmethod
    def describe(cls, config):
        """The numbers a run is judged by, one line each: resolution in wall units, Reynolds numbers, the scales of
        velocity, length and time, and the wall type."""
        u_tau = cls.subdomain.u_tau(config.Re_tau)
        u0 = cls.subdomain.u0
        y_plus = (np.arange(config.H) + 0.5) * u_tau / config.visc
        u_bulk = float(np.sum(log_law(y_plus)) * u_tau / config.H)
        Re_centre = u0 * config.H / config.visc
        rows = [('wall units per node spacing', '%.2f' % (u_tau / config.visc)),
                ('Re_tau', '%.2f' % config.Re_tau),
                ('Re of the centre-line velocity and H', '%.2f' % Re_centre),
                ('Re of the bulk velocity and H', '%.2f' % (u_bulk * config.H / config.visc)),
                ('viscosity', '%e' % config.visc),
                ('bulk velocity of the log law', '%e' % u_bulk),
                ('friction velocity', '%e' % u_tau),
                ('Kolmogorov length (node spacings)', '%e' % (2.0 * config.H / Re_centre ** 0.75)),
                ('acceleration', '%e' % cls.force(config)),
                ('large-eddy turnover time (steps)', '%d' % (2.0 * config.H / u0)),
                ('flow-through time (steps)', '%d' % cls.t_flow(config)),
                ('H / u_tau (steps)', '%d' % cls.t_char(config)),
                ('wall nodes', cls.subdomain.wall_bc.__name__)]
        return ['%-40s %s' % row for row in rows]

    def __init__(self, config):
        super(ChannelSim, self).__init__(config)
        self.add_body_force((0.0, 0.0, self.force(config)))
        for line in self.describe(config):
            config.logger.info(line)
        if getattr(config, 'stats_snapshots', 0) > 0:
            self.stat_buf_size = int(config.stats_snapshots)

    def _stats_dir(self):
        return os.path.join(self.config.output, 'reyn_stats') if self.config.output else None

    def before_main_loop(self, runner):
        self.prepare_reynolds_stats(runner, axis='x')
        path = self._stats_dir()
        if path and not os.path.isdir(path):
            os.makedirs(path, exist_ok=True)

    def after_step(self, runner):
        start = getattr(self.config, 'stats_after', -1)
        if self.iteration < (start if start >= 0 else 2 * self.t_flow(self.config)):
            return                                          # transients
        phase = self.iteration % SAMPLE_EVERY
        if phase == SAMPLE_EVERY - 1:
            self.need_fields_flag = True                    # the next step stores rho and v
        elif phase == 0:
            stats = self.collect_reynolds_stats(runner)
            path = self._stats_dir()
            if stats is not None and path:
                np.savez(os.path.join(path, 'stats_%s.%s' % (runner._spec.id, self.iteration)), **stats)


if __name__ == '__main__':
    LBSimulationController(ChannelSim, EqualSubdomainsGeometry3D).run()
