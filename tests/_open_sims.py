"""Simulations for the runner-level tests of the do-nothing outlet and the full-slip wall.  The first is the set-up of
the reference's tests/gpu/do_nothing_node.py (full-way bounce-back walls on y, a regularized-velocity inlet, NTDoNothing
on the last column, everything moving at 0.05 to begin with); framed_sim() lays the same channels out in any frame of
tests/_faces.py (tests/test_gpu_faces.py); test-only."""
import numpy as np

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish.lb_base import LBForcedSim
from sailfish.lb_single import LBFluidSim
from sailfish import node_type as nt
from sailfish.node_type import NTDoNothing, NTFullBBWall, NTRegularizedVelocity, NTSlip
from sailfish.subdomain import Subdomain2D, Subdomain3D
from sailfish.sym import D2Q9, D3Q19


class OpenChannelSubdomain(Subdomain2D):
    u_in = 0.05

    def boundary_conditions(self, hx, hy):
        wall = (hy == 0) | (hy == self.gy - 1)
        self.set_node(wall, NTFullBBWall)
        self.set_node(~wall & (hx == 0), NTRegularizedVelocity((self.u_in, 0.0)))
        self.set_node(~wall & (hx == self.gx - 1), NTDoNothing)

    def initial_conditions(self, sim, hx, hy):
        sim.rho[:] = 1.0
        sim.vx[:] = self.u_in


class OpenChannelSim(LBFluidSim):
    subdomain = OpenChannelSubdomain


class OpenDuctSubdomain(Subdomain3D):
    u_in = 0.04

    def boundary_conditions(self, hx, hy, hz):
        wall = (hy == 0) | (hy == self.gy - 1)
        self.set_node(wall, NTFullBBWall)
        self.set_node(~wall & (hz == 0), NTRegularizedVelocity((0.0, 0.0, self.u_in)))
        self.set_node(~wall & (hz == self.gz - 1), NTDoNothing)

    def initial_conditions(self, sim, hx, hy, hz):
        sim.rho[:] = 1.0
        sim.vz[:] = self.u_in


class OpenDuctSim(LBFluidSim):
    """Flow along z between walls on y, periodic along x; the outlet is a z face."""
    subdomain = OpenDuctSubdomain

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'periodic_x': True})


class SlipChannelSubdomain(Subdomain2D):
    """Flow along x between two full-slip walls: nothing holds the fluid back.  `u0`: the uniform initial velocity."""
    u0 = 0.0

    def boundary_conditions(self, hx, hy):
        self.set_node(hy == 0, NTSlip(orientation=D2Q9.vec_to_dir([0, 1])))
        self.set_node(hy == self.gy - 1, NTSlip(orientation=D2Q9.vec_to_dir([0, -1])))

    def initial_conditions(self, sim, hx, hy):
        sim.rho[:] = 1.0
        sim.vx[:] = self.u0


class SlipChannelSim(LBFluidSim, LBForcedSim):
    subdomain = SlipChannelSubdomain
    accel = 1e-5

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'periodic_x': True})

    def __init__(self, config):
        super(SlipChannelSim, self).__init__(config)
        if self.accel:
            self.add_body_force((self.accel, 0.0))


class SlipDuctSubdomain(Subdomain3D):
    def boundary_conditions(self, hx, hy, hz):
        self.set_node(hy == 0, NTSlip(orientation=D3Q19.vec_to_dir([0, 1, 0])))
        self.set_node(hy == self.gy - 1, NTSlip(orientation=D3Q19.vec_to_dir([0, -1, 0])))

    def initial_conditions(self, sim, hx, hy, hz):
        sim.rho[:] = 1.0


class SlipDuctSim(LBFluidSim, LBForcedSim):
    subdomain = SlipDuctSubdomain
    accel = 1e-5

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'periodic_x': True, 'periodic_z': True})

    def __init__(self, config):
        super(SlipDuctSim, self).__init__(config)
        self.add_body_force((self.accel, 0.0, 0.0))


def framed_sim(dim, frame, walls='fullbb', inlet='NTRegularizedVelocity', outlet='NTDoNothing', force=None, u0=0.04):
    """A channel in a frame of tests/_faces.py: (flow axis, sign, wall axis) in 3-D, (flow axis, sign) in 2-D; the third
    axis of a duct is periodic.
    walls: 'fullbb' or 'slip' (NTSlip with its inward normal; where the channel is open the two ends of a slip wall are
    full-way nodes: a slip node exchanges populations with its neighbours along the wall, which would be ghost nodes there).
    inlet / outlet: node-type names for the upstream / downstream face of the flow axis -- a velocity inlet gets u0 along
    the flow, a density outlet 1.0, the outflow kinds nothing (the host finds their orientation) -- or None: periodic along the flow, driven by
    the body force `force` along it.  Everything moves at u0 along the flow to begin with."""
    grid = D2Q9 if dim == 2 else D3Q19
    fa, fs = frame[0], frame[1]
    fb = frame[2] if dim == 3 else 1 - fa
    is_open = inlet is not None

    def unit(axis, size):
        v = [0.0] * dim if isinstance(size, float) else [0] * dim
        v[axis] = size
        return v

    class FramedSubdomain(Subdomain2D if dim == 2 else Subdomain3D):
        def boundary_conditions(self, *h):
            g = (self.gx, self.gy) + ((self.gz,) if dim == 3 else ())
            along = h[fa] if fs > 0 else g[fa] - 1 - h[fa]
            across = h[fb]
            low, high = across == 0, across == g[fb] - 1
            ends = (along == 0) | (along == g[fa] - 1)
            if walls == 'slip':
                full = (low | high) & ends if is_open else np.zeros_like(low)
                self.set_node(low & ~full, NTSlip(orientation=grid.vec_to_dir(unit(fb, 1))))
                self.set_node(high & ~full, NTSlip(orientation=grid.vec_to_dir(unit(fb, -1))))
                self.set_node(full, NTFullBBWall)
            else:
                self.set_node(low | high, NTFullBBWall)
            if is_open:
                free = ~(low | high)
                self.set_node(free & (along == 0), getattr(nt, inlet)(tuple(unit(fa, fs * u0))))
                cls = getattr(nt, outlet)
                if cls.value_name == 'density':
                    self.set_node(free & (along == g[fa] - 1), cls(1.0))
                else:                   # (the orientation is found by the host: Subdomain.detect_orientation)
                    self.set_node(free & (along == g[fa] - 1), cls)

        def initial_conditions(self, sim, *h):
            sim.rho[:] = 1.0
            (sim.vx, sim.vy, sim.vz if dim == 3 else None)[fa][:] = fs * u0

    bases = (LBFluidSim, LBForcedSim) if force else (LBFluidSim,)

    class FramedSim(*bases):
        subdomain = FramedSubdomain

        # the periodic axes, as configuration keywords (the tests pass their configuration as a whole)
        periodic_cfg = dict([('periodic_' + 'xyz'[3 - fa - fb], True)] if dim == 3 else [],
                            **({} if is_open else {'periodic_' + 'xyz'[fa]: True}))

        @classmethod
        def update_defaults(cls, defaults):
            defaults.update(cls.periodic_cfg)

        def __init__(self, config):
            super(FramedSim, self).__init__(config)
            if force:
                self.add_body_force(tuple(unit(fa, fs * float(force))))

    return FramedSim
