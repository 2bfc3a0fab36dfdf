#!/usr/bin/env python3
"""Generate tests/golden/flow_stats.npz from the reference's own host functions: sailfish/util.py vorticity(),
kinetic_energy() and enstrophy() evaluated on the initial field of its examples/turbulence/kida_vortex.py
(max_v = 0.05, no shift) on a 20 x 12 x 9 box, in single and in double precision.

Runs ONLY in the authoring container (needs the reference next to the repository, see tools/ref_shim.py); the fixture
is data (inputs + expected outputs).  Nothing in tests/ or the product reads the reference at run time.

    PYTHONPATH=tools python tools/capture_stats_goldens.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: F401  (installs import stubs, puts the reference on sys.path)

import numpy as np

from sailfish import util as ref_util  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'flow_stats.npz')
SIZE = (20, 12, 9)       # nx, ny, nz
MAX_V = 0.05


def kida(size, max_v, dtype):
    """The field KidaSubdomain.initial_conditions() assigns: formed in double, rounded by the assignment to the
    simulation's fields."""
    nx, ny, nz = size
    hz, hy, hx = np.mgrid[0:nz, 0:ny, 0:nx]
    x = hx * np.pi * 2.0 / nx
    y = hy * np.pi * 2.0 / ny
    z = hz * np.pi * 2.0 / nz
    sin, cos = np.sin, np.cos
    v = np.zeros((3, nz, ny, nx), dtype=dtype)
    v[0] = max_v * sin(x) * (cos(3 * y) * cos(z) - cos(y) * cos(3 * z))
    v[1] = max_v * sin(y) * (cos(3 * z) * cos(x) - cos(z) * cos(3 * x))
    v[2] = max_v * sin(z) * (cos(3 * x) * cos(y) - cos(x) * cos(3 * y))
    return v


def main():
    out = {'size': np.array(SIZE), 'max_v': np.float64(MAX_V)}
    for tag, dtype in (('f32', np.float32), ('f64', np.float64)):
        v = kida(SIZE, MAX_V, dtype)
        w = ref_util.vorticity(v, 1.0)
        assert w.dtype == dtype
        out['v_' + tag] = v
        out['vorticity_' + tag] = w
        out['kinetic_energy_' + tag] = np.float64(ref_util.kinetic_energy(v))
        out['enstrophy_' + tag] = np.float64(ref_util.enstrophy(v, 1.0))
        print(tag, 'kinetic energy %.12g  enstrophy %.12g' % (out['kinetic_energy_' + tag], out['enstrophy_' + tag]))
    np.savez_compressed(OUT, **out)
    print('written', os.path.normpath(OUT), os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
