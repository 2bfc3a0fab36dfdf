"""Immersed boundary markers on the GPU (csrc/slf_ibm.hip behind slf_ibm_*; lb_single.LBIBMFluidSim with
IBMSubdomainRunner) against the numpy twin (tests/_ibm_twin.py), bit for bit; repeatability, step plans, restore; a ring of
stiff markers in a driven channel; the refusals of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

from sailfish_amd import geo as geo_mod
from sailfish_amd import hipabi
from tests import _accf, _ibm, _lat
from tests._ibm_twin import IbmTwinBox

pytestmark = pytest.mark.gpu

UNIFORM = [0.7e-5, -0.4e-5, 0.9e-5]


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def box_pair(backend, name, pattern, precision, model):
    """(twin, device box with markers, index of the marker that is outside) on the shapes of the issue: D2Q9 32 x 16 between
    full-way walls on y, D3Q19 16 x 12 x 10 fully periodic."""
    grid, size = _accf.GRIDS[name], _ibm.SHAPES[name]
    dim = grid.dim
    walls = 'full' if dim == 2 else None
    pos, ref, k, out = _ibm.marker_set(size)
    kw = dict(accel=UNIFORM[:dim], accel_field=True)
    desc, periodic, map_fn = _accf.box_desc(grid, size, pattern, precision, 'guo', walls, 1, model=model, **kw)
    nmap = None if map_fn is None else map_fn(desc)
    # the twin's fluid step is BGK; under MRT it is not called (the fluid fields are taken from the device, see below)
    d_twin = desc if model == 'bgk' else _accf.box_desc(grid, size, pattern, precision, 'guo', walls, 1, **kw)[0]
    twin = _accf.start(IbmTwinBox(d_twin, periodic, nmap, pos, ref, k), size, dim)
    gpu = _ibm.BoxWithMarkers(backend, desc, periodic, nmap, pos, ref, k)
    _accf.start(gpu.box, size, dim)
    return twin, gpu, out


def fetch_v(gpu):
    _, v = gpu.box.fetch_fields()
    return v


# ---- 1. parity with the twin --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('model', ['bgk', 'mrt'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', ['D2Q9', 'D3Q19'])
def test_parity_with_the_twin(backend, name, precision, pattern, model):
    """Positions as uploaded, the accumulator after spread, the field after gather (NaN in every ghost and padding entry,
    before and after), positions / accumulator / field / `outside` after every one of 20 steps.  BGK: populations, rho and
    v after every step too -- the whole state.  MRT: the twin's fluid step is BGK only (tests/_accf_twin.py), so the twin
    takes the velocity field of every step from the device and the marker arithmetic is held against it bit for bit; the
    MRT sweep itself is the unchanged ACCF sweep (tests/test_gpu_accel_field.py)."""
    twin, gpu, out = box_pair(backend, name, pattern, precision, model)
    dim = twin.dim
    try:
        assert same(gpu.positions(), twin.positions())
        n_nan = np.isnan(twin.accel_field).sum()
        assert n_nan == twin.accel_field.size - dim * np.prod(_ibm.SHAPES[name])
        for step in range(20):
            twin.spread()
            twin.gather()
            if step == 0:
                gpu.markers.backend.ibm_spread(gpu.box.module, gpu.markers.n, gpu.markers.origin, gpu.markers.gpu_position,
                                               gpu.markers.gpu_ref_position, gpu.markers.gpu_stiffness, gpu.markers.gpu_acc,
                                               gpu.box.stream)
                assert same(gpu.acc(), twin.acc) and twin.acc.any()
                assert not gpu.field()[~np.isnan(twin.accel_field)].any()           # nothing converted yet
                gpu.markers.backend.ibm_gather(gpu.box.module, gpu.markers.n, gpu.markers.origin, gpu.markers.gpu_position,
                                               gpu.markers.gpu_acc, gpu.box.stream)
                field = gpu.field()
                assert same(field, twin.accel_field) and np.isnan(field).sum() == n_nan
                assert np.nanmax(np.abs(field)) > 0
            else:
                gpu.front()
            gpu.box.step(save_macro=True)
            if model == 'bgk':
                super(IbmTwinBox, twin).step(save_macro=True)
                assert same(gpu.box.real_view(gpu.box.get_dist()), twin.real_view(twin.current_dist())), step
                rho, v = gpu.box.fetch_fields()
                assert same(gpu.box.real_view(rho), twin.real_view(twin.rho)), step
                for k in range(dim):
                    assert same(gpu.box.real_view(v[k]), twin.real_view(twin.v[k])), step
            else:
                for k, c in enumerate(fetch_v(gpu)):
                    twin.v[k][...] = c
            gpu.back()
            twin.clear_and_advect()
            assert same(gpu.positions(), twin.positions()), step
            assert gpu.outside() == twin.outside == 1
            assert same(gpu.acc(), twin.acc) and not twin.acc.any()
            field = gpu.field()
            assert same(field, twin.accel_field) and np.isnan(field).sum() == n_nan and not np.nansum(np.abs(field))
        start = _ibm.marker_set(_ibm.SHAPES[name])[0].astype(twin.dtype)
        moved = np.abs(twin.positions() - start).max(axis=1) > 0
        assert not moved[out] and moved.sum() == _ibm.N_MARKERS - 1          # the marker whose stencil leaves stays put
        assert np.all(np.isfinite(gpu.box.real_view(gpu.box.get_dist())))
    finally:
        gpu.release()


# ---- 2. the runner: repeatability, step plans, restore, and the twin again ---------------------------------------------------

def run_channel(name, pattern, precision, model, steps=20, **over):
    size = _ibm.SHAPES[name]
    dim = len(size)
    pos, ref, k, _ = _ibm.marker_set(size)
    sim = _ibm.channel_sim(dim, pos, ref, k, UNIFORM[:dim], walls=dim == 2, start=_accf.start_fields(size, dim))
    geo = geo_mod.LBGeometry2D if dim == 2 else geo_mod.LBGeometry3D
    cfg = _ibm.channel_cfg(size, pattern, precision, model, **over)
    if dim == 3:
        cfg.update(periodic_y=True)
    return _lat.run_gpu(sim, cfg, steps, geo)


def state(ctrl):
    r = ctrl.runners[0]
    return [r._debug_get_dist(), r.particle_positions(), r._sim.rho] + list(r._sim.v)


CASES = [('D2Q9', 'AB', 'single', 'bgk'), ('D2Q9', 'AA', 'double', 'mrt'), ('D3Q19', 'AA', 'single', 'bgk'),
         ('D3Q19', 'AB', 'double', 'mrt')]


@pytest.mark.parametrize('name,pattern,precision,model', CASES)
def test_two_runs_are_bit_identical_and_step_plans_change_nothing(name, pattern, precision, model):
    a = run_channel(name, pattern, precision, model)
    r = a.runners[0]
    assert type(r).__name__ == 'IBMSubdomainRunner' and r._desc.accel_field == 1 and r._markers.n == _ibm.N_MARKERS
    assert r.ibm_outside == 1
    assert same(r._sim.particle_positions, r.particle_positions())             # refreshed with the fields of the last step
    assert np.abs(r.particle_positions() - _ibm.marker_set(_ibm.SHAPES[name])[0]).max() > 1e-3
    b = run_channel(name, pattern, precision, model)
    c = run_channel(name, pattern, precision, model, hip_step_plans=False)
    assert a.runners[0]._step_plans.plans and not c.runners[0]._step_plans.plans
    for x, y, z in zip(state(a), state(b), state(c)):
        assert same(x, y) and same(x, z)
    assert np.all(np.isfinite(state(a)[1]))


@pytest.mark.parametrize('name,pattern,precision,model', CASES)
def test_restored_run_equals_the_straight_run(name, pattern, precision, model, tmp_path):
    straight = run_channel(name, pattern, precision, model)
    ck = str(tmp_path / 'ck')
    run_channel(name, pattern, precision, model, steps=7, checkpoint_file=ck, final_checkpoint=True)
    cp = [f for f in os.listdir(str(tmp_path)) if f.startswith('ck') and f.endswith('.cpoint.npz')]
    assert len(cp) == 1
    restored = run_channel(name, pattern, precision, model,
                           restore_from=os.path.join(str(tmp_path), cp[0][:-len('.0.cpoint.npz')]))
    assert restored.runners[0]._sim.iteration == 20
    for x, y in zip(state(straight), state(restored)):
        assert same(x, y)


# ---- 3. physics: a ring of stiff markers in a driven channel ---------------------------------------------------------------------
# 48 x 26 nodes between full-way walls (24 fluid rows), periodic along x, visc = 0.1, acceleration 2e-5 along x, 300 steps
# from rest; a ring of 24 markers of radius 5 around the centre of the channel, stiffness 0.05, each tied to where it
# starts.  The marker speed is the mean over the markers of |v_p|, v_p the velocity field the last sweep stored, interpolated
# at the positions the markers had during that sweep (float64 on the host, the same function for device and twin: the
# positions themselves move by less than their single-precision spacing per step).  Without markers the centreline of the
# channel would be at about a H^2 / (8 visc) (1 - exp(-pi^2 visc T / H^2)) = 2e-5 x 576 / 0.8 x 0.402 = 5.8e-3.
# The double-precision twin on the CPU gives 2.43e-5 (the number is printed by the test and recorded in DESIGN.md §9h).
RING = dict(size=(48, 26), visc=0.1, accel=(2e-5, 0.0), steps=300, n=24, radius=5.0, stiffness=0.05)


def ring_markers():
    pos = np.array(_ibm.ring((23.5, 12.5), RING['radius'], RING['n']))
    return pos, pos.copy(), np.full(RING['n'], RING['stiffness'])


def ring_twin(precision='double'):
    grid = _accf.GRIDS['D2Q9']
    pos, ref, k = ring_markers()
    desc, periodic, map_fn = _accf.box_desc(grid, RING['size'], 'AB', precision, 'guo', 'full', 1, accel=list(RING['accel']),
                                            accel_field=True, visc=RING['visc'])
    return desc, periodic, map_fn(desc), pos, ref, k


def marker_speed(pos, vx, vy):
    """Mean |v_p|: bilinear interpolation of the velocity over the real nodes (arrays [ny, nx]) at pos [n, 2], float64."""
    pos = pos.astype(np.float64)
    i0 = np.floor(pos).astype(int)
    vp = np.zeros((2, len(pos)))
    for oy in (0, 1):
        for ox in (0, 1):
            w = (1.0 - np.abs(pos[:, 0] - (i0[:, 0] + ox))) * (1.0 - np.abs(pos[:, 1] - (i0[:, 1] + oy)))
            for k, c in enumerate((vx, vy)):
                vp[k] += w * c.astype(np.float64)[i0[:, 1] + oy, i0[:, 0] + ox]
    return float(np.sqrt((vp ** 2).sum(axis=0)).mean())


@pytest.fixture(scope='module')
def ring_reference():
    """The double-precision twin, computed once: (positions during the last sweep, vx, vy of that sweep, final positions)."""
    desc, periodic, nmap, pos, ref, k = ring_twin()
    t = IbmTwinBox(desc, periodic, nmap, pos, ref, k)
    shape = tuple(reversed(RING['size']))
    t.set_fields(np.ones(shape), [np.zeros(shape)] * 2)
    t.initial_conditions()
    for _ in range(RING['steps'] - 1):
        t.step()
    during = t.positions()
    t.step()
    return during, np.array(t.real_view(t.v[0])), np.array(t.real_view(t.v[1])), t.positions()


@pytest.mark.parametrize('precision', ['single', 'double'])
def test_ring_of_stiff_markers_holds_the_fluid(backend, precision, ring_reference):
    desc, periodic, nmap, pos, ref, k = ring_twin(precision)
    gpu = _ibm.BoxWithMarkers(backend, desc, periodic, nmap, pos, ref, k)
    try:
        shape = tuple(reversed(RING['size']))
        gpu.box.set_fields(np.ones(shape), [np.zeros(shape)] * 2)
        gpu.box.initial_conditions()
        for _ in range(RING['steps'] - 1):
            gpu.step()
        during = gpu.positions()
        gpu.step()
        after = gpu.positions()
        _, v = gpu.box.fetch_fields()
        vx, vy = [np.array(gpu.box.real_view(c)) for c in v]
    finally:
        gpu.release()
    twin_speed = marker_speed(*ring_reference[:3])
    got = marker_speed(during, vx, vy)
    h = RING['size'][1] - 2
    free = RING['accel'][0] * h * h / (8.0 * RING['visc']) * (1.0 - np.exp(-np.pi ** 2 * RING['visc'] * RING['steps'] / (h * h)))
    far = float(np.abs(vx[h // 2, 1]))                         # the centreline away from the ring (printed only)
    print('ring, %s: marker speed %.6e (twin, double: %.6e), unobstructed centreline %.6e, centreline far from the ring %.6e'
          % (precision, got, twin_speed, free, far))
    assert twin_speed < 0.01 * free                           # "well below": two orders of magnitude in the twin itself
    assert got <= 2.0 * twin_speed
    if precision == 'double':
        assert same(during, ring_reference[0]) and same(after, ring_reference[3])
        assert same(vx, ring_reference[1]) and same(vy, ring_reference[2])


# ---- 4. refusals at the C ABI -----------------------------------------------------------------------------------------------------

def test_c_abi_refuses_what_the_bind_program_lists(backend):
    lib = backend._lib
    grid, size = _accf.GRIDS['D3Q19'], (16, 5, 4)
    P = ctypes.c_void_p
    origin = (ctypes.c_int32 * 3)(0, 0, 0)
    plain, periodic, _ = _accf.box_desc(grid, size, 'AB', 'single', 'guo', accel=[1e-5, 0.0, 0.0])
    from sailfish_amd.box import BoxSim
    s = BoxSim(backend, plain, periodic=periodic)
    try:
        a = P(s.gpu_rho)
        n = ctypes.c_size_t()
        assert lib.slf_ibm_workspace_bytes(s.module.handle, ctypes.byref(n)) == 1 and b'accel_field' in lib.slf_last_error()
        assert lib.slf_ibm_spread(s.module.handle, 4, origin, a, a, a, a, s.stream.handle) == 1
        assert b'slf_ibm_spread' in lib.slf_last_error() and b'accel_field' in lib.slf_last_error()
    finally:
        s.release()
    desc, periodic, _ = _accf.box_desc(grid, size, 'AB', 'single', 'guo', accel_field=True)
    s = BoxSim(backend, desc, periodic=periodic)                         # created with the flag, no field set yet
    try:
        a = P(s.gpu_rho)
        assert lib.slf_ibm_workspace_bytes(s.module.handle, ctypes.byref(n)) == 0
        assert n.value == 3 * 8 * desc.arr_nx * desc.arr_ny * desc.arr_nz
        assert lib.slf_ibm_gather(s.module.handle, 4, origin, a, a, s.stream.handle) == 1
        assert b'slf_module_set_accel_field' in lib.slf_last_error()
        field = np.zeros((3,) + s.shape, dtype=s.dtype)
        addr = backend.alloc_buf(like=field)
        backend.set_accel_field(s.module, addr)
        for count, word in ((0, b'positive'), (-3, b'positive'), ((1 << 24) + 1, b'2^24')):
            assert lib.slf_ibm_gather(s.module.handle, count, origin, a, a, s.stream.handle) == 1
            assert word in lib.slf_last_error()
        assert lib.slf_ibm_gather(s.module.handle, 4, None, a, a, s.stream.handle) == 1 and b'origin' in lib.slf_last_error()
        assert lib.slf_ibm_gather(s.module.handle, 4, origin, None, a, s.stream.handle) == 1 and b'pos is NULL' in lib.slf_last_error()
        assert lib.slf_ibm_spread(s.module.handle, 4, origin, a, a, None, a, s.stream.handle) == 1
        assert b'stiffness is NULL' in lib.slf_last_error()
        assert lib.slf_ibm_clear_and_advect(s.module.handle, 4, origin, a, a, None, a, a, None, a, s.stream.handle) == 1
        assert b'vz is NULL' in lib.slf_last_error()
        assert lib.slf_ibm_spread(None, 4, origin, a, a, a, a, s.stream.handle) == 1
        s.sync()
        backend.from_buf(addr, field)
        assert not field.any()                                           # and nothing was launched
        backend.free_buf(addr)
    finally:
        s.release()
    from sailfish_amd import sym
    from sailfish_amd.box import make_box_desc
    module = backend.build(make_box_desc(sym.D3Q15, size, precision='single', access_pattern='AB', visc=0.02,
                                         periodic_fused=[1, 1, 1]))            # a module only: nothing is launched on it
    addr = backend.alloc_buf(size=256)
    assert module.desc.lattice == hipabi.SLF_D3Q15
    assert lib.slf_ibm_gather(module.handle, 4, origin, P(addr), P(addr), None) == 3          # SLF_ERR_UNSUPPORTED
    assert b'D3Q15' in lib.slf_last_error()
    backend.free_buf(addr)
