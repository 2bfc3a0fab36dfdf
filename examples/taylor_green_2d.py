#!/usr/bin/env python
"""Decaying Taylor-Green vortices in a doubly periodic box, D2Q9 (cf. sailfish's examples/taylor_green_2d.py).

With kx = 2 pi lambda_x / nx, ky = 2 pi lambda_y / ny and k^2 = kx^2 + ky^2 the velocity field

    u_x = -max_v (ky / k) sin(ky y) cos(kx x) d(t),    u_y = max_v (kx / k) sin(kx x) cos(ky y) d(t),    d(t) = exp(-visc k^2 t)

solves the incompressible Navier-Stokes equations together with the pressure field
p0 - (rho / 4) max_v^2 ((ky / k)^2 cos(2 kx x) + (kx / k)^2 cos(2 ky y)) d(t)^2, which the lattice-Boltzmann equation of state
(p = rho cs^2) turns into the density of solution() below.  Every --err_every steps the run prints

    iteration, relative velocity error (L2, against the analytic solution), largest speed of the simulation and of the
    solution, largest density of the simulation and of the solution, relative density error

evaluated on the whole domain: each subdomain compares its own nodes, at their global coordinates, and prints a line of
its own.  examples/four_rolls_mill.py adds the body force that keeps the vortices from decaying."""
from __future__ import print_function

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root (the `sailfish` alias)

from sailfish.controller import LBSimulationController
from sailfish.geo import EqualSubdomainsGeometry2D
from sailfish.lb_single import LBFluidSim
from sailfish.subdomain import Subdomain2D


class TaylorGreenSubdomain(Subdomain2D):
    def boundary_conditions(self, hx, hy):
        pass

    def initial_conditions(self, sim, hx, hy):
        mach = self.config.max_v / math.sqrt(sim.grid.cssq)
        sim.rho[:], sim.vx[:], sim.vy[:] = self.solution(self.config, hx, hy, self.gx, self.gy, 0, mach)

    @classmethod
    def get_k(cls, config, gx, gy):
        """(kx, ky, k^2, k): lattice coordinates times kx, ky run over lambda_x, lambda_y periods of 2 pi."""
        kx = 2.0 * np.pi * config.lambda_x / gx
        ky = 2.0 * np.pi * config.lambda_y / gy
        ksq = kx * kx + ky * ky
        return kx, ky, ksq, math.sqrt(ksq)

    @classmethod
    def solution(cls, config, hx, hy, gx, gy, t, Ma):
        """(rho, vx, vy) of the analytic solution at the nodes (hx, hy) of a gx x gy domain after t steps."""
        kx, ky, ksq, k = cls.get_k(config, gx, gy)
        decay = np.exp(-config.visc * ksq * t)
        amp = config.max_v * decay / k
        vx = -amp * ky * np.sin(ky * hy) * np.cos(kx * hx)
        vy = amp * kx * np.sin(kx * hx) * np.cos(ky * hy)
        rho = 1.0 - 0.25 * Ma * Ma / ksq * (ky * ky * np.cos(2.0 * kx * hx) + kx * kx * np.cos(2.0 * ky * hy)) * decay * decay
        return rho, vx, vy


class TaylorGreenSim(LBFluidSim):
    subdomain = TaylorGreenSubdomain

    @classmethod
    def update_defaults(cls, defaults):
        defaults.update({'periodic_x': True, 'periodic_y': True, 'lat_nx': 256, 'lat_ny': 256, 'visc': 0.001})

    @classmethod
    def add_options(cls, group, dim):
        group.add_argument('--max_v', type=float, default=0.01, help='Maximum velocity in LB units.')
        group.add_argument('--lambda_x', type=int, default=1)
        group.add_argument('--lambda_y', type=int, default=1)
        group.add_argument('--err_every', type=int, default=100, help='How often to evaluate the error.')

    def reference_solution(self, hx, hy, nx, ny, iteration, Ma):
        """(four_rolls_mill overrides this: its solution does not decay)"""
        return self.subdomain.solution(self.config, hx, hy, nx, ny, iteration, Ma)

    def errors(self, runner):
        """(relative velocity error, top speed, top speed of the solution, top density, top density of the solution,
        relative density error) of this subdomain's fields against the solution at iteration self.iteration."""
        vx, vy, rho = [np.asarray(a, dtype=np.float64) for a in (self.vx, self.vy, self.rho)]
        hx, hy = runner._subdomain._get_mgrid()          # global coordinates of this subdomain's nodes
        nx, ny = runner._global_size
        mach = self.config.max_v / math.sqrt(self.grid.cssq)
        ref_rho, ref_vx, ref_vy = self.reference_solution(hx, hy, nx, ny, self.iteration, mach)
        err = math.sqrt(np.sum((ref_vx - vx) ** 2 + (ref_vy - vy) ** 2) / np.sum(ref_vx ** 2 + ref_vy ** 2))
        rho_err = np.linalg.norm(ref_rho - rho) / np.linalg.norm(ref_rho)
        return (err, np.sqrt(vx * vx + vy * vy).max(), np.sqrt(ref_vx ** 2 + ref_vy ** 2).max(), rho.max(), ref_rho.max(),
                rho_err)

    def after_step(self, runner):
        every = self.config.err_every
        if self.iteration % every == every - 1:
            self.need_sync_flag = True           # the next step stores the fields
        elif self.iteration % every == 0:
            print(self.iteration, *self.errors(runner))


if __name__ == '__main__':
    LBSimulationController(TaylorGreenSim, EqualSubdomainsGeometry2D).run()
