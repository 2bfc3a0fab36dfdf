"""Set-ups shared by the tests of the acceleration field (tests/test_accf_twin.py, tests/test_gpu_accel_field.py): box
descriptors with or without a field, channels with full-way or half-way walls on the two y faces, seeded start fields.
Test-only."""
import numpy as np

from sailfish_amd import hipabi, sym
from sailfish_amd.box import make_box_desc
from tests import _geometry as geo

GRIDS = {'D2Q9': sym.D2Q9, 'D3Q19': sym.D3Q19}


def walled_map(grid, desc, kind):
    """Walls on the faces y = 1 and y = max, x (and z) periodic: kind 'full' = full-way bounce-back, 'half' = half-way
    bounce-back with link tags (the tags see the periodic neighbours)."""
    m = geo.empty_map(desc)
    ny, nx = desc.lat_ny - 2, desc.lat_nx - 2
    zs = list(range(1, desc.lat_nz - 1)) if grid.dim == 3 else [0]
    t = geo.T_FULLBB if kind == 'full' else geo.T_HALFBB
    for z in zs:
        m[z, 1, 1:nx + 1] = geo.encode(t)
        m[z, ny, 1:nx + 1] = geo.encode(t)
    if kind == 'full':
        return m
    mm = m.copy()
    mm[:, :, 0] = mm[:, :, nx]
    mm[:, :, nx + 1] = mm[:, :, 1]
    if grid.dim == 3:
        nz = desc.lat_nz - 2
        mm[0] = mm[nz]
        mm[nz + 1] = mm[1]
    for z in zs:
        for y in (1, ny):
            for x in range(1, nx + 1):
                m[z, y, x] = geo.encode(geo.T_HALFBB, orientation=geo.link_tags(grid, mm, z, y, x))
    return m


def box_desc(grid, size, pattern, precision, force, walls=None, fused=1, accel=None, accel_field=False, model='bgk',
             visc=0.02):
    """(descriptor, periodic axes, node-map builder or None).  walls: None (fully periodic), 'full', 'half' (y faces)."""
    dim = grid.dim
    periodic = [True] * 3 if walls is None else [True, False, True]
    periodic = tuple(periodic[:dim]) + (False,) * (3 - dim)
    kw = {}
    if walls is not None:
        kw = dict(fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, use_link_tags=True)
    desc = make_box_desc(grid, size, model=model, precision=precision, access_pattern=pattern, visc=visc,
                         periodic_fused=[int(fused and p) for p in periodic], accel=accel, accel_field=accel_field, **kw)
    desc.force_implementation = hipabi.SLF_FORCE_EDM if force == 'edm' else hipabi.SLF_FORCE_GUO
    return desc, periodic, (None if walls is None else (lambda d: walled_map(grid, d, walls)))


def start_fields(size, dim, seed=77):
    """rho = 1 + 1e-2 U, |v| < 0.03, different at every node and in every component."""
    rng = np.random.RandomState(seed)
    shape = tuple(reversed(size))
    return 1.0 + 1e-2 * rng.rand(*shape), [0.03 * (2.0 * rng.rand(*shape) - 1.0) for _ in range(dim)]


def start(sim, size, dim, node_map_fn=None, seed=77):
    rho, v = start_fields(size, dim, seed)
    sim.set_fields(rho, v)
    sim.initial_conditions()
    return sim
