"""NTWallTMS (Tamm-Mott-Smith wall) on the GPU against its numpy twin (tests/_tms_twin.py, itself held against the
reference's sympy objects by tests/test_tms_twin.py), and through the host stack against itself across decompositions
and addressing modes.

Every box case: random non-equilibrium populations, 5 steps -- both parities of the in-place pattern run, and what a TMS
node stores feeds its next target state -- with every slot of every real node compared after every step, and the density
and velocity the last step saved.

Where the order of the kernels' operations is restated exactly the results are bit-identical and equality is asserted
(-ffp-contract=off, every operation a correctly rounded IEEE one on both sides): the BGK collision in its three density
forms, with and without the Guo force, restated in numpy; and MRT and the subgrid model, whose collision of a node comes
from the C oracle, one node at a time -- the oracle is the kernels' arithmetic contract (the same
order, the same fused multiply-adds), around which the twin puts its boundary steps.  Every such case also prints how
far it is from the twin against four times what the twin differs from itself in the next wider format over the same run
(tests/test_gpu_elbm.py::_twin_error; without a wider format, 16 eps per step).  The entropic collision
(tests/_elbm_twin.collide) evaluates logarithms, another library's on each side: there the bound is four times what the
twin with ln x differs from the twin with log2(x) ln 2 over the same run, with a floor of 1e-13 relative."""
import os
import subprocess
import sys

import numpy as np
import pytest

from sailfish_amd import hipabi, sym
from sailfish_amd.box import BoxSim, make_box_desc
from tests import _elbm_twin as etw
from tests import _tms_twin as tw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPE = {'single': np.float32, 'double': np.float64}
STEPS = 5
VISC = 0.02
# dense type ids of the hand-encoded maps, orientation | type (2 type bits, no parameter bits)
TYPE_KIND = [hipabi.SLF_NK_FLUID, hipabi.SLF_NK_GHOST, hipabi.SLF_NK_WALL_TMS]
T_FLUID, T_GHOST, T_TMS = range(3)
NT_BITS = (2, 0, 0)
# name -> (grid, (lat_nx, lat_ny[, lat_nz]) with ghosts, wall-normal axes)
GRIDS = {
    'd2-y': (sym.D2Q9, (66, 6), (1,)),             # walls normal to y
    'd2-x': (sym.D2Q9, (10, 66), (0,)),            # walls normal to x: the TMS nodes are the first and last lanes of a row
    'd3-yz': (sym.D3Q19, (66, 6, 5), (1, 2)),      # walls normal to y and to z
    'd3-z': (sym.D3Q19, (130, 5, 4), (2,)),        # walls normal to z, rows of two waves
    'd3-x': (sym.D3Q19, (12, 8, 7), (0,)),         # walls normal to x
    'duct': (sym.D3Q19, (34, 10, 8), (1, 2)),      # four faces: edge nodes with many missing links
}
ACCEL = {2: [1e-4, -5e-5], 3: [1e-4, -5e-5, 7e-5]}
FORM = {'compressible': hipabi.SLF_DENSITY_COMPRESSIBLE, 'incompressible': hipabi.SLF_DENSITY_INCOMPRESSIBLE,
        'roundoff': hipabi.SLF_DENSITY_ROUNDOFF}


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def _wider(dtype):
    if dtype is np.float32:
        return np.float64
    return np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else None


def geometry(grid, lat_xyz, wall_axes, use_tags):
    """TMS nodes on the first and last real layer of every wall axis, the other axes periodic.  Over the lattice
    [(lat_nz,) lat_ny, lat_nx]: (tms mask, orientation words, missing [Q, lattice], periodic per lattice axis)."""
    lat = tuple(reversed(lat_xyz))
    nd = len(lat)
    idx = np.indices(lat)
    real = np.ones(lat, dtype=bool)
    for k in range(nd):
        real &= (idx[k] >= 1) & (idx[k] <= lat[k] - 2)
    tms = np.zeros(lat, dtype=bool)
    for ax in wall_axes:
        k = nd - 1 - ax
        tms |= real & ((idx[k] == 1) | (idx[k] == lat[k] - 2))
    words = np.zeros(lat, dtype=np.int64)
    if use_tags:
        for i in range(1, grid.Q):                      # bit i - 1: direction i points to a wet node
            wet = np.ones(lat, dtype=bool)
            for ax in wall_axes:
                k = nd - 1 - ax
                c = idx[k] + grid.basis[i][ax]
                wet &= (c >= 1) & (c <= lat[k] - 2)
            words[tms & wet] |= 1 << (i - 1)
        missing = tw.missing_from_tags(grid, words)
    else:
        assert len(wall_axes) == 1
        ax = wall_axes[0]
        k = nd - 1 - ax
        n = [0] * grid.dim
        n[ax] = 1
        words[real & (idx[k] == 1)] = grid.vec_to_dir(n)
        n[ax] = -1
        words[real & (idx[k] == lat[k] - 2)] = grid.vec_to_dir(n)
        missing = tw.missing_from_orientation(grid, words)
    periodic = [ax not in wall_axes for ax in range(grid.dim)]
    return tms, words, missing, periodic


def populations(grid, lat, dtype, roundoff, seed=11):
    """rho in [0.9, 1.1], |u| <= 0.1, plus a non-equilibrium part of 5 %; the ghost layer holds zeros."""
    rng = np.random.RandomState(seed)
    rho = rng.uniform(0.9, 1.1, lat)
    v = [rng.uniform(-0.1, 0.1, lat) / np.sqrt(grid.dim) for _ in range(grid.dim)] + [np.zeros(lat)] * (3 - grid.dim)
    f = tw.feq(grid, rho, rho, v) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (grid.Q,) + lat))
    if roundoff:
        f = f - np.array([float(w) for w in grid.weights]).reshape((grid.Q,) + (1,) * len(lat))
    real = np.ones(lat, dtype=bool)
    for k, c in enumerate(np.indices(lat)):
        real &= (c >= 1) & (c <= lat[k] - 2)
    return np.where(real[None], f, 0.0).astype(dtype)


def oracle_collide(desc, grid, precision):
    """The collision of a wet node from the C oracle (orc_node_update on a fluid node: moments, relaxation, force), one
    node at a time, in the precision asked for (4 / 8), whatever the arrays' format."""
    from oracle import oracle

    def collide(f, rho, v, rho0):
        out = np.empty_like(f)
        vo = [np.zeros_like(rho) for _ in range(3)]
        for n in range(f.shape[1]):
            g, _, vv = oracle.node_update(desc, hipabi.SLF_NK_FLUID, 0, None, f[:, n].astype(np.float64), precision=precision)
            out[:, n] = g
            for d in range(3):
                vo[d][n] = vv[d]
        return out, vo
    return collide


def elbm_collide(grid, incompressible=False, log2=False):
    def collide(f, rho, v, rho0):
        r = etw.collide(grid, f, VISC, incompressible=incompressible, log2=log2)
        assert r['ok'].all()
        return r['f'], list(r['v'])
    return collide


def run_case(backend, name, pattern, precision, model='bgk', form='compressible', force=True, tags=True, fused=True,
             subgrid=False):
    """GPU and twin side by side.  Returns (exact, err, tol, twin): are all compared values bit-identical; the largest
    difference; the twin's own error in the next wider format (None where there is none: the oracle's collision in double
    precision; elbm: how far the twin with another logarithm drifts from it)."""
    grid, lat_xyz, wall_axes = GRIDS[name]
    dtype = DTYPE[precision]
    tms, words, missing, periodic = geometry(grid, lat_xyz, wall_axes, tags)
    lat = tms.shape
    accel = ACCEL[grid.dim] if force else None
    size = tuple(n - 2 for n in lat_xyz)
    per3 = periodic + [False] * (3 - grid.dim)
    desc = make_box_desc(grid, size, model=model, precision=precision, access_pattern=pattern, visc=VISC,
                         periodic_fused=[int(p and fused) for p in per3], fluid_only=False, accel=accel,
                         incompressible=FORM[form], type_kind=TYPE_KIND, nt_bits=NT_BITS, use_link_tags=tags,
                         subgrid='les-smagorinsky' if subgrid else None, smagorinsky_const=0.17)
    node_map = np.full((desc.arr_nz, desc.arr_ny, desc.arr_nx), T_GHOST, dtype=np.uint32)
    code = np.where(tms, (words << NT_BITS[0]) | T_TMS, T_FLUID).astype(np.uint32)
    real = np.ones(lat, dtype=bool)
    for k, c in enumerate(np.indices(lat)):
        real &= (c >= 1) & (c <= lat[k] - 2)
    code = np.where(real, code, T_GHOST).astype(np.uint32)
    node_map[:, :, :lat[-1]] = code.reshape((desc.arr_nz, desc.arr_ny, lat[-1]))
    s = BoxSim(backend, desc, periodic=tuple(per3), node_map=node_map, alpha_field=False if model == 'elbm' else None)
    backend.set_iteration(0)           # (the backend is shared: the kernels' step parity starts with this box)
    f0 = populations(grid, lat, dtype, form == 'roundoff')
    full = np.zeros((grid.Q,) + s.shape, dtype=dtype)
    full[..., :lat[-1]] = f0.reshape((grid.Q,) + s.shape[:-1] + (lat[-1],))
    for which in range(len(s.gpu_dist)):
        s.set_dist(full, which)

    def twin(dt, log2=False):
        if model == 'elbm':
            col = elbm_collide(grid, form == 'incompressible', log2)
        elif model == 'mrt' or subgrid:
            if dt not in (np.float32, np.float64):
                return None
            col = oracle_collide(desc, grid, 4 if dt is np.float32 and dt is dtype else 8)
        else:
            col = None
        return tw.TmsTwin(grid, f0.astype(dt), tms, missing, VISC, periodic, pattern=pattern, density=form, accel=accel,
                          collide=col)
    t = twin(dtype)
    wide_dt = _wider(dtype)
    if model == 'elbm':        # the yardstick of tests/test_gpu_elbm.py: the same twin with ln x formed as log2(x) ln 2
        wide = twin(dtype, log2=True)
    else:
        wide = twin(wide_dt) if wide_dt is not None else None
    exact, err, tol = True, 0.0, 0.0

    def compare(got, ref, refw):
        nonlocal exact, err, tol
        exact = exact and np.array_equal(got, ref)
        err = max(err, float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)))))
        if refw is not None:
            tol = max(tol, float(np.max(np.abs(ref.astype(refw.dtype) - refw))))

    rsl = (Ellipsis,) + tuple(slice(1, n - 1) for n in lat)
    for step in range(STEPS):
        s.step(save_macro=(step == STEPS - 1))
        t.step()
        if wide is not None:
            wide.step()
        got = s.get_dist()[..., :lat[-1]].reshape((grid.Q,) + lat)
        compare(got[rsl], t.current()[rsl], wide.current()[rsl] if wide is not None else None)
    assert backend.poll_invalid(s.module, s.stream) is None
    g_rho, g_v = s.fetch_fields()
    fields = [(g_rho, t.rho, wide.rho if wide is not None else None)]
    fields += [(g_v[d], t.v[d], wide.v[d] if wide is not None else None) for d in range(grid.dim)]
    for got, ref, refw in fields:
        got = got[..., :lat[-1]].reshape(lat)
        compare(got[rsl[1:]], ref[rsl[1:]], refw[rsl[1:]] if refw is not None else None)
    assert t.missing.any() and np.isfinite(t.current()[rsl]).all()
    s.release()
    if wide is None:
        tol = None
    return exact, err, tol, t


def _check(res, label, dtype, exact_expected):
    exact, err, tol, _ = res
    bound = 4 * tol if tol is not None else STEPS * 16 * float(np.finfo(dtype).eps)
    print('%s: bit-identical %s, |gpu - twin| %.3e, bound %.3e' % (label, exact, err, bound))
    assert err <= bound, (label, err, bound)
    if exact_expected:
        assert exact, label


# ---- BGK, the order restated exactly: bit-identical -------------------------------------------------------------------

SHAPE_CASES = [(n, tags) for n in sorted(GRIDS) for tags in ((True, False) if len(GRIDS[n][2]) == 1 else (True,))]


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name,tags', SHAPE_CASES, ids=['%s-%s' % (n, 'tags' if t else 'orientation') for n, t in SHAPE_CASES])
def test_shapes_bgk_guo(backend, name, tags, pattern, precision):
    res = run_case(backend, name, pattern, precision, tags=tags)
    _check(res, '%s %s %s' % (name, pattern, precision), DTYPE[precision], True)


# (compressible with the Guo force: test_shapes_bgk_guo)
FORM_CASES = [(f, g) for f in ('compressible', 'incompressible', 'roundoff') for g in (False, True)
              if not (f == 'compressible' and g)]


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('form,force', FORM_CASES, ids=['%s-%s' % (f, 'guo' if g else 'noforce') for f, g in FORM_CASES])
@pytest.mark.parametrize('name', ['d2-y', 'd3-z'])
def test_density_forms(backend, name, form, force, pattern, precision):
    res = run_case(backend, name, pattern, precision, form=form, force=force)
    _check(res, '%s %s %s %s %s' % (name, form, force, pattern, precision), DTYPE[precision], True)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name', ['d2-y', 'd3-z', 'd3-x'])
def test_periodic_through_the_ghost_layers(backend, name, pattern):
    """The periodic axes served by the ghost-layer kernels instead of the in-sweep wrap."""
    res = run_case(backend, name, pattern, 'single', fused=False)
    _check(res, '%s %s ghost-layer' % (name, pattern), np.float32, True)


def test_forced_boundary_level(backend, monkeypatch):
    """SLF_BC_LEVEL=2 is accepted by a module with TMS nodes and changes nothing in it: the per-node kernels exist at level
    2 only, and the slot sweep of a TMS module is its level-2 instantiation whatever the level says -- there is no lower
    level with TMS code to be forced up from.  The case is the duct's in-place round-off run with the variable set."""
    monkeypatch.setenv('SLF_BC_LEVEL', '2')
    res = run_case(backend, 'duct', 'AA', 'single', form='roundoff')
    _check(res, 'duct AA single roundoff, SLF_BC_LEVEL=2', np.float32, True)


# ---- collisions from elsewhere: the oracle's (bit-identical), the entropic twin's (within the spread of two logarithms) --------------------------------------------------

@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name,force', [('d2-y', True), ('d3-x', True), ('duct', False)])
def test_mrt(backend, name, force, pattern, precision):
    res = run_case(backend, name, pattern, precision, model='mrt', force=force)
    _check(res, '%s mrt %s %s' % (name, pattern, precision), DTYPE[precision], True)


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_subgrid_les_smagorinsky(backend, pattern, precision):
    res = run_case(backend, 'd3-z', pattern, precision, subgrid=True)
    _check(res, 'd3-z les %s %s' % (pattern, precision), DTYPE[precision], True)


@pytest.mark.parametrize('name', ['d2-y', 'd3-yz'])
def test_elbm(backend, name):
    """The entropic collision between TMS walls: the twin's boundary steps around tests/_elbm_twin.collide (no alpha
    array: every Newton iteration starts from 2 on both sides).  Two equally valid implementations of the collision -- the
    twin with ln x and the twin with log2(x) ln 2 -- drift apart by `spread` over the run; the kernels, a third, may be
    four times that from the twin (the factor of every other case of this file; floor: 1e-13 relative)."""
    exact, err, spread, t = run_case(backend, name, 'AA', 'double', model='elbm', force=False)
    scale = float(np.max(np.abs(t.current())))
    bound = max(4 * spread, 1e-13 * scale)
    print('%s elbm: |gpu - twin| %.3e, spread of the two twins %.3e, bound %.3e' % (name, err, spread, bound))
    assert err <= bound, (err, bound)


# ---- the reference's own test set-up -----------------------------------------------------------------------------------

def test_reference_test_setup_two_steps(backend):
    """The set-up of the reference's tests/gpu/tms.py: D2Q9, 64 x 16, double precision, two-copy pattern, visc 1/12, TMS
    walls on the two y rims, all populations zero except those of one wall node, which are the reference's.  Run for two
    steps against the twin.  Its own expectation for the first step -- the unknown populations bounced back before the
    target state is formed -- is not asserted: the templates take the target state from the populations as loaded
    (boundary.mako:635), and what is loaded equals the bounced-back values only from the second step on, when the node's
    own store has put them there (tests/test_tms_twin.py); after hand-set populations the first step differs, and that
    first step is all the reference's test looks at.  (The reference also switches propagation off; the library has no
    such switch, and the node in question is compared after it has streamed.)"""
    grid = sym.D2Q9
    start = {(0, 0): 0.4745, (1, 0): 0.1179, (-1, 0): 0.1045, (0, -1): 0.1809, (-1, -1): 0.03613, (1, -1): 0.00946,
             (1, 1): 0.02946, (0, 1): 0.1110, (-1, 1): 0.02613}
    lat_xyz = (66, 18)
    tms, words, missing, periodic = geometry(grid, lat_xyz, (1,), True)
    lat = tms.shape
    visc = 1.0 / 12.0
    desc = make_box_desc(grid, (64, 16), precision='double', access_pattern='AB', visc=visc, periodic_fused=[1, 0, 0],
                         fluid_only=False, type_kind=TYPE_KIND, nt_bits=NT_BITS, use_link_tags=True)
    real = np.ones(lat, dtype=bool)
    for k, c in enumerate(np.indices(lat)):
        real &= (c >= 1) & (c <= lat[k] - 2)
    code = np.where(real, np.where(tms, (words << NT_BITS[0]) | T_TMS, T_FLUID), T_GHOST).astype(np.uint32)
    node_map = np.full((desc.arr_nz, desc.arr_ny, desc.arr_nx), T_GHOST, dtype=np.uint32)
    node_map[0, :, :lat[1]] = code
    s = BoxSim(backend, desc, periodic=(True, False, False), node_map=node_map)
    backend.set_iteration(0)
    # every node starts from the rest state (a node without mass divides by zero); the wall node (x, y) = (16, 1) of the
    # reference's test -- (17, 1) with the ghost layer -- carries its populations
    rho = np.ones(lat)
    zero = np.zeros(lat)
    f0 = tw.feq(grid, rho, rho, [zero, zero, zero])
    f0[:, ~real] = 0.0
    for vec, val in start.items():
        f0[grid.vec_idx(vec), 1, 17] = val
    full = np.zeros((grid.Q,) + s.shape)
    full[:, 0, :, :lat[1]] = f0
    for which in range(2):
        s.set_dist(full, which)
    t = tw.TmsTwin(grid, f0, tms, missing, visc, periodic, pattern='AB')
    rsl = (Ellipsis,) + tuple(slice(1, n - 1) for n in lat)
    for step in range(2):
        s.step(save_macro=False)
        t.step()
        got = s.get_dist()[:, 0, :, :lat[1]]
        assert np.array_equal(got[rsl], t.current()[rsl]), step
    s.release()


# ---- through the host stack --------------------------------------------------------------------------------------------

CHANNEL = dict(H=8, Re_tau=20.0, wall='tms')


def _channel(steps, **kw):
    from examples.turbulence.channel_flow import ChannelSim
    from tests.test_gpu_runner import merged_gpu, run_gpu
    cfg = dict(CHANNEL)
    cfg.update(kw)
    ctrl = run_gpu(ChannelSim, None, 3, cfg, steps)
    out = {'rho': merged_gpu(ctrl, 'rho')}
    for d in range(3):
        out['v%d' % d] = merged_gpu(ctrl, 'v%d' % d)
    return ctrl, out


def test_channel_one_subdomain_against_two():
    """The channel script's classes, 60 steps: one subdomain against two along z and two along y, TMS nodes on the seam:
    density and velocity bit-identical (the rule of the 1-vs-N regressions of tests/test_gpu_runner.py)."""
    ctrl, one = _channel(60)
    assert all(np.isfinite(a).all() for a in one.values())
    assert np.ptp(one['v2']) > 0 and np.ptp(one['v0']) > 0
    kinds = list(ctrl.runners[0]._desc.type_kind[:ctrl.runners[0]._desc.n_types])
    assert hipabi.SLF_NK_WALL_TMS in kinds
    for axis in ('z', 'y'):
        _, two = _channel(60, subdomains=2, conn_axis=axis)
        for key in sorted(one):
            assert np.array_equal(one[key], two[key]), (axis, key)


def test_channel_reynolds_stats():
    from examples.turbulence.channel_flow import ChannelSim
    from tests.test_gpu_runner import run_gpu

    got = {}

    class Probe(ChannelSim):
        stat_buf_size = 1            # one snapshot fills the device ring: the first collection returns the profiles

        def after_step(self, runner):
            if self.iteration == 39:
                self.need_fields_flag = True
            elif self.iteration == 40:
                got['stats'] = self.collect_reynolds_stats(runner)

    ctrl = run_gpu(Probe, None, 3, dict(CHANNEL), 41)
    stats = got['stats']
    assert stats is not None
    nx = ctrl.runners[0]._spec.size[0]
    assert nx == 2 * CHANNEL['H'] + 2
    assert list(stats['iters']) == [40]
    for key, val in stats.items():
        arr = np.asarray(val)
        if key != 'iters' and arr.ndim:
            assert arr.shape[-1] == nx, key
            assert np.isfinite(arr).all(), key


def _indirect_fields(steps, pattern, sim='DuctSim', **kw):
    from tests import _tms_sims as S
    from tests.test_gpu_runner import merged_gpu, run_gpu
    ctrl = run_gpu(getattr(S, sim), None, 3, dict(S.CFG, access_pattern=pattern, **kw), steps)
    out = {'rho': merged_gpu(ctrl, 'rho')}
    for d in range(3):
        out['v%d' % d] = merged_gpu(ctrl, 'v%d' % d)
    for r in ctrl.runners:
        r.release()
    return out


# what runs: bgk / mrt -> slot_sweep_kernel<.., 2, true>; roundoff, les, elbm -> sweep_kernel<.., INDIRECT, .., TMS> (the slot
# sweep does not serve them); roundoff with the Guo force in place is the channel script's own configuration
INDIRECT_VARIANTS = {'bgk': {}, 'mrt': dict(model='mrt'), 'roundoff': dict(minimize_roundoff=True),
                     'les': dict(subgrid='les-smagorinsky', smagorinsky_const=0.17), 'elbm': dict(model='elbm')}


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('variant', sorted(INDIRECT_VARIANTS))
def test_indirect_addressing(variant, pattern, precision):
    """A duct of TMS walls with a block inside: storage for the active nodes only against the dense arrays -- the numbers
    live elsewhere, they are the same numbers."""
    kw = dict(INDIRECT_VARIANTS[variant], precision=precision)
    sim = 'DuctSimNoForce' if variant == 'elbm' else 'DuctSim'       # (no body forces under the entropic collision)
    dense = _indirect_fields(21, pattern, sim=sim, **kw)
    sparse = _indirect_fields(21, pattern, sim=sim, node_addressing='indirect', **kw)
    assert np.ptp(dense['v0']) > 0
    for key in sorted(dense):
        assert np.array_equal(dense[key], sparse[key], equal_nan=True), key


def test_indirect_addressing_per_node_kernel(tmp_path):
    """The per-node indirect sweep (SLF_INDIRECT_SLOTS=0 is read once per process: a child) against the dense arrays."""
    env = dict(os.environ, SLF_INDIRECT_SLOTS='0')
    res = subprocess.run([sys.executable, os.path.join(HERE, '_tms_sims.py'), str(tmp_path)], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, env=env, timeout=300)
    out = res.stdout.decode('utf-8', 'replace')
    assert res.returncode == 0, out
    assert 'SLF_INDIRECT_SLOTS=0' in out
    for pattern in ('AB', 'AA'):
        dense = _indirect_fields(21, pattern, precision='single')
        for key in sorted(dense):
            assert np.array_equal(dense[key], np.load(os.path.join(str(tmp_path), '%s.%s.npy' % (pattern, key))),
                                  equal_nan=True), (pattern, key)
