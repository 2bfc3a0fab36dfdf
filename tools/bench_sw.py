#!/usr/bin/env python3
"""Rate of the shallow-water sweep beside the D2Q9 BGK per-node sweep (profiles/sw/README.md).

One process times one model on a periodic, single-precision, two-copy box through LBSimulationController:

    python tools/bench_sw.py --model sw                        LBFreeSurface, this tree
    SLF_VARIANT=0 python tools/bench_sw.py --model bgk --tree PARENT
                                                               LBFluidSim BGK of the tree at PARENT (a checkout of the parent
                                                               commit with its library built), held to the per-node kernels

The run is `warmup` untimed blocks, then `blocks` timed blocks of `steps` steps, then one more block that is left out: the
run's last step copies the fields to the host, which is not the sweep's time (at 4096^2 it takes a third off that block's
rate).  The runner synchronises the device at the end of every block (--perf_stats_every) and logs the block's rate, which
is read back from the log.  Printed: one JSON line with the
rate of every block in MLUPS (million node updates per second), their median and their spread (max - min) / median.  To
compare two models, alternate the two commands in one session and take the spread of the baseline's blocks as the margin.
Needs a GPU: without one the backend raises."""
import argparse
import json
import logging
import os
import re
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=['sw', 'bgk'], required=True)
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the repository whose sailfish_amd runs (default: the one this file is in)')
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=400, help='steps per timed block')
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1, help='untimed blocks in front')
    ap.add_argument('--access_pattern', default='AB')
    ap.add_argument('--precision', default='single')
    ap.add_argument('--backends', default=None,
                    help='rehearsal only: a CPU test backend (tests._sw_backend) to walk the script without a GPU; the '
                         'rates it prints mean nothing')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

    from sailfish_amd.controller import LBSimulationController
    from sailfish_amd.geo import LBGeometry2D
    from sailfish_amd import lb_single
    from sailfish_amd.subdomain import Subdomain2D

    class Box(Subdomain2D):
        def boundary_conditions(self, hx, hy):
            pass

        def initial_conditions(self, sim, hx, hy):
            sim.rho[:] = 1.0 + 0.01 * np.cos(2.0 * np.pi * hx / self.gx) * np.cos(2.0 * np.pi * hy / self.gy)

    base = lb_single.LBFreeSurface if args.model == 'sw' else lb_single.LBFluidSim

    class Sim(base):
        subdomain = Box

    rates = []

    class Capture(logging.Handler):
        def emit(self, record):
            m = re.search(r'speed:([0-9.]+) MLUPS', record.getMessage())
            if m:
                rates.append(float(m.group(1)))

    total = (args.warmup + args.blocks + 1) * args.steps
    cfg = dict(lat_nx=args.size, lat_ny=args.size, periodic_x=True, periodic_y=True, precision=args.precision,
               access_pattern=args.access_pattern, visc=0.01, max_iters=total, perf_stats_every=args.steps, output='',
               grid='D2Q9', model='bgk')
    if args.model == 'sw':
        cfg['gravity'] = 0.05
    if args.backends:
        cfg.update(backends=args.backends, gpus=[0])
    logging.getLogger('sailfish').addHandler(Capture())
    ctrl = LBSimulationController(Sim, LBGeometry2D, default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    if len(rates) != args.warmup + args.blocks + 1:
        raise RuntimeError('expected %d blocks, the log gave %d rates' % (args.warmup + args.blocks + 1, len(rates)))
    timed = rates[args.warmup:-1]
    med = float(np.median(timed))
    print(json.dumps(dict(model=args.model, tree=os.path.abspath(args.tree), size=args.size, steps=args.steps,
                          access_pattern=args.access_pattern, precision=args.precision,
                          variant=os.environ.get('SLF_VARIANT'), blocks_mlups=timed, last_block_mlups=rates[-1], median_mlups=med,
                          spread=(max(timed) - min(timed)) / med, bytes_per_node=72 if args.precision == 'single' else 144,
                          gbytes_per_s=med * 1e6 * (72 if args.precision == 'single' else 144) * 1e-9, rehearsal=bool(args.backends))))


if __name__ == '__main__':
    main()
