#!/usr/bin/env python3
"""Force-object fixture from the reference's own host code (authoring container only): what its
Subdomain.get_fo_distributions() (sailfish/subdomain.py:734-770) returns for an interior bounding box around the
cylinder of examples/cylinder.py (2-D channel) and around the sphere of examples/sphere_3d.py (3-D duct); no link of
either box leaves the domain.  Output: tests/golden/force_objects.npz with, per case <c>,

    <c>_cfg_keys / <c>_cfg_vals   the lattice size (lat_nx, lat_ny[, lat_nz])
    <c>_start, <c>_end            the bounding box
    <c>_vis_map                   the reference's node types of the real nodes (uint8)
    <c>_dirs                      the direction indices of the returned dict, ascending
    <c>_d<i>                      [dim, n] coordinates of direction i: the returned tuple, stacked in its order

    python tools/capture_force_objects.py
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: F401
sys.path.insert(2, '/root/reference/examples')

import numpy as np

from capture_geometry import OUT, base_config
from sailfish.backend_dummy import DummyBackend
from sailfish.controller import LBGeometryProcessor
from sailfish.io import LBOutput
from sailfish.lb_base import ForceObject
from sailfish.subdomain_runner import SubdomainRunner

CASES = {
    'cylinder': dict(module='cylinder', sim='CylinderSimulation', dim=2, start=(13, 8), end=(27, 22),
                     cfg=dict(lat_nx=48, lat_ny=30, visc=0.1, vertical=False, force_implementation='guo')),
    'sphere': dict(module='sphere_3d', sim='SphereSimulation', dim=3, start=(6, 4, 4), end=(15, 12, 12),
                   cfg=dict(lat_nx=20, lat_ny=16, lat_nz=16, visc=0.05, force_implementation='guo')),
}


def run_case(case):
    mod = importlib.import_module(case['module'])
    sim_cls = getattr(mod, case['sim'])
    cfg = base_config(case['dim'], **case['cfg'])
    sim_cls.modify_config(cfg)
    from sailfish import geo as ref_geo
    geo = getattr(ref_geo, 'LBGeometry2D' if case['dim'] == 2 else 'LBGeometry3D')(cfg)
    specs = geo.subdomains()
    for s in specs:
        s.set_actual_size(1)
    spec = LBGeometryProcessor(specs, case['dim'], geo.gsize).transform(cfg)[0]
    sim = sim_cls(cfg)
    runner = SubdomainRunner(sim, spec, output=LBOutput(cfg, spec.id), backend=DummyBackend(), quit_event=None)
    runner._init_geometry()
    fo = ForceObject(case['start'], case['end'])
    sim.add_force_oject(fo)
    return runner._subdomain, runner._subdomain.get_fo_distributions(fo)


def main():
    out = {}
    for name, case in CASES.items():
        sub, dists = run_case(case)
        keys = sorted(k for k in case['cfg'] if k.startswith('lat_n'))
        out[name + '_cfg_keys'] = np.array(keys)
        out[name + '_cfg_vals'] = np.array([case['cfg'][k] for k in keys])
        out[name + '_start'] = np.array(case['start'])
        out[name + '_end'] = np.array(case['end'])
        out[name + '_vis_map'] = np.array(sub._type_vis_map, dtype=np.uint8)
        out[name + '_dirs'] = np.array(sorted(dists), dtype=np.int64)
        for i, locs in dists.items():
            out['%s_d%d' % (name, i)] = np.stack([np.asarray(x, dtype=np.int64) for x in locs])
        print('captured', name, 'directions', sorted(dists), 'links', sum(l[0].size for l in dists.values()))
    np.savez_compressed(os.path.join(OUT, 'force_objects.npz'), **out)


if __name__ == '__main__':
    main()
