"""D3Q15 and D3Q27 on the GPU (csrc/slf_lat.hip) against the numpy twin (tests/_lat_twin.py, itself held against the
reference's sympy objects and the CPU oracle by tests/test_lat_twin.py) and against themselves across configurations.
The comparisons are bit for bit: the kernels are built with -ffp-contract=off and a step has no transcendental function,
so the twin does every operation the kernels do, in the same order and format (the standard of tests/test_gpu_sc3.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sailfish_amd import hipabi, io, sym
from sailfish_amd.geo import LBGeometry3D
from tests import _kat, _lat
from tests import _lat_twin as tw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = _lat.LATTICES


def _against_twin(sim, cfg, steps, geo=LBGeometry3D, fields=False):
    """The populations of every wet node after `steps` steps: GPU == twin, bit for bit.  Returns the GPU's."""
    ctrl = _lat.run_gpu(sim, cfg, steps, geo)
    t = tw.TwinGroup(sim, geo, cfg).run(steps)
    wet = np.isin(t.merged('kind'), tw.WET)
    got, want = _lat.merged(ctrl, 'dist'), t.merged('dist')
    assert wet.any() and np.all(np.isfinite(want[:, wet]))
    diff = int(np.count_nonzero(got[:, wet] != want[:, wet]))
    if diff:
        err = float(np.max(np.abs(got[:, wet].astype(np.float64) - want[:, wet].astype(np.float64))))
        print('%d of %d wet slots differ, largest difference %.3e' % (diff, want[:, wet].size, err))
    assert diff == 0
    if fields:      # the fields the last step stored (its density and the velocity its collision used)
        assert np.array_equal(_lat.merged(ctrl, 'rho')[wet], t.merged('rho')[wet])
        for d in range(3):
            assert np.array_equal(_lat.merged(ctrl, 'v%d' % d)[wet], t.merged('v%d' % d)[wet])
    return got, wet


# ---- one collision --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', LATTICES)
def test_one_collision_against_the_twin(golden_dir, name, precision):
    """A periodic 66 x 4 x 3 box every node of which carries the same populations is invariant under streaming: one step
    leaves every node with the post-collision state.  The populations of the fixture (off equilibrium by up to 5 %), with a
    Guo force; a 66-node row is one wave plus two nodes."""
    from sailfish_amd.backend_hip import HIPBackend
    from sailfish_amd.box import BoxSim, make_box_desc

    class Opt(object):
        pass
    grid, R = sym.lookup_grid(name), _lat.DTYPE[precision]
    g = np.load(os.path.join(golden_dir, 'arith_lat_%s.npz' % name))
    desc = make_box_desc(grid, (66, 4, 3), precision=precision, access_pattern='AB', visc=float(g['visc']),
                         periodic_fused=[1, 1, 1], accel=list(_lat.ACCEL))
    box = BoxSim(HIPBackend(Opt(), 0), desc, periodic=(True, True, True))
    assert box.Q == grid.Q and box.k_pair is None and name in box.pair_refused       # no pair sweep on these lattices
    try:
        for k in range(0, len(g['f']), 4):
            f0 = g['f'][k].astype(R)
            box.set_dist(np.broadcast_to(f0[:, None, None, None], (grid.Q,) + box.shape), which=0)
            box.iteration = 0
            box.step()
            out = box.real_view(box.get_dist(1)).reshape(grid.Q, -1)
            assert np.all(out == out[:, :1])                   # every node did the same arithmetic
            rho, v = tw.macro(grid, f0[:, None], False, R)
            want, _ = tw.relax(grid, f0[:, None], rho, v, R(1.0 / desc.tau), R(3.0 * (1.0 - 0.5 / desc.tau)), False,
                               [R(a) for a in _lat.ACCEL], False, R)
            assert np.array_equal(out[:, 0], want[:, 0]), (k, np.max(np.abs(out[:, 0] - want[:, 0])))
            assert not np.array_equal(want[:, 0], f0)
    finally:
        box.release()


# ---- whole steps ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('force', [None, 'guo', 'edm'], ids=['noforce', 'guo', 'edm'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name', LATTICES)
def test_whole_steps_short_rows(name, pattern, precision, force):
    """20 and 21 steps on a periodic 66 x 6 x 5 box from a smooth random state (after 21 in-place steps the arrays hold the
    populations un-streamed)."""
    box = dict(size=(66, 6, 5), walls=None, force=force)
    for steps in (20, 21):
        sim, cfg = _lat.case(name, box, pattern=pattern, precision=precision)
        _against_twin(sim, cfg, steps, fields=True)


@pytest.mark.parametrize('name', LATTICES)
def test_whole_steps_incompressible(name):
    sim, cfg = _lat.case(name, dict(size=(66, 6, 5), walls=None, force='guo'), pattern='AA', precision='single', incompressible=True)
    got, _ = _against_twin(sim, cfg, 21, fields=True)
    other, _ = _against_twin(*_lat.case(name, dict(size=(66, 6, 5), walls=None, force='guo'), pattern='AA', precision='single'), steps=21)
    assert not np.array_equal(got, other)


# rows of three waves (wave-edge words on both sides of the middle one); rows cut into segments: 1030 nodes for every
# instantiation, 800 for the 768-thread workgroups of D3Q27 / f32, 600 for the 512-thread ones of double precision
LONG_ROWS = [((130, 4, 3), 'single', 'AB'), ((130, 4, 3), 'single', 'AA'), ((130, 4, 3), 'double', 'AB'), ((130, 4, 3), 'double', 'AA'),
             ((1030, 3, 3), 'single', 'AB'), ((800, 3, 3), 'single', 'AA'), ((600, 3, 3), 'double', 'AB'), ((600, 3, 3), 'double', 'AA')]


@pytest.mark.parametrize('size,precision,pattern', LONG_ROWS, ids=['%d-%s-%s' % (s[0], p, a) for s, p, a in LONG_ROWS])
@pytest.mark.parametrize('name', LATTICES)
def test_whole_steps_long_rows(name, size, precision, pattern):
    steps = 5 if size[0] > 130 else 21
    sim, cfg = _lat.case(name, dict(size=size, walls=None, force='guo'), pattern=pattern, precision=precision)
    _against_twin(sim, cfg, steps)


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('box', [_lat.WALL_BOX, _lat.CHANNEL], ids=['wall-box-guo', 'channel-halfway-edm'])
@pytest.mark.parametrize('name', LATTICES)
def test_walls(name, box, pattern, precision):
    for steps in (20, 21):
        sim, cfg = _lat.case(name, box, pattern=pattern, precision=precision)
        _against_twin(sim, cfg, steps, fields=True)


@pytest.mark.parametrize('name', LATTICES)
def test_relaxation_disabled_only_streams(name):
    sim, cfg = _lat.case(name, dict(size=(20, 6, 5), walls=None, force=None), pattern='AB', precision='single')
    sim.modify_config = classmethod(lambda cls, config: setattr(config, 'relaxation_enabled', False))
    got, _ = _against_twin(sim, cfg, 5)
    start = tw.TwinGroup(sim, LBGeometry3D, cfg).merged('dist')
    assert np.ptp(start) > 0
    grid = sym.lookup_grid(name)
    for i, e in enumerate(grid.basis):
        assert np.array_equal(got[i], np.roll(start[i], tuple(5 * c for c in reversed(e)), axis=(0, 1, 2)))


# ---- the reference's known-answer runs on D3Q15 -----------------------------------------------------------------------------

def test_d3q15_propagation_known_answers(tmp_path):
    """Every D3Q15 run of tests/golden/propagation_kat.json (SingleBlockPeriodicQ15Test of the reference's
    regtest/subdomains/3d_propagation.py), through the controller as tests/test_gpu_kat.py runs the others."""
    from sailfish_amd.controller import LBSimulationController
    runs = [(i, r) for i, r in _kat.all_runs() if r['grid'] == 'D3Q15']
    assert len(runs) >= 1
    for n, (rid, run) in enumerate(runs):
        for fused in (True, False):
            sim_cls, geo_cls, cfg, grid = _kat.make_classes(run)
            assert grid is sym.D3Q15
            out = str(tmp_path / ('kat%d%d' % (n, fused)))
            cfg.update(hip_fused_periodic=fused, output=out, every=1, debug_dump_dists=True, quiet=True, perf_stats_every=0,
                       check_invalid_results_host=False)
            relax = cfg.pop('relaxation_enabled')
            sim_cls.modify_config = classmethod(lambda cls, config, relax=relax: setattr(config, 'relaxation_enabled', relax))
            LBSimulationController(sim_cls, geo_cls, default_config=cfg).run(ignore_cmdline=True)
            digits = io.filename_iter_digits(run['max_iters'])
            assert len(run['expects']) > 0
            _kat.check(run, grid, lambda sid, it: np.load(io.dists_filename(out, digits, sid, it))['arr_0'])


# ---- bit for bit between configurations -----------------------------------------------------------------------------------

@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('box', [_lat.WALL_BOX, _lat.PERIODIC_BOX], ids=['wall-box', 'periodic-box'])
@pytest.mark.parametrize('name', LATTICES)
def test_decompositions_equal_one_subdomain(name, box, pattern):
    """Two x slabs, 2 x 2 x 2 blocks (faces, edges and corners) and -- the periodic box -- the ghost-layer periodic kernels,
    each equal to one subdomain wrapped inside the sweep, on every wet slot."""
    steps = 10
    sim, cfg = _lat.case(name, box, pattern=pattern, precision='single')
    one, wet = _against_twin(sim, cfg, steps)

    def same(ctrl, what, n):
        assert len(ctrl.runners) == n, what
        assert np.array_equal(_lat.merged(ctrl, 'dist')[:, wet], one[:, wet]), what
    from sailfish_amd.geo import EqualSubdomainsGeometry3D
    variants = [True] + ([False] if box['walls'] is None else [])
    for fused in variants:
        c = dict(cfg, hip_fused_periodic=fused)
        if not fused:
            same(_lat.run_gpu(sim, c, steps), 'ghost-layer periodicity', 1)
        same(_lat.run_gpu(sim, dict(c, subdomains=2, conn_axis='x'), steps, EqualSubdomainsGeometry3D), 'two x slabs', 2)
        same(_lat.run_gpu(sim, c, steps, _lat.block_geometry([[10], [6], [5]])), '2 x 2 x 2 blocks', 8)


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('box', [_lat.WALL_BOX, _lat.CHANNEL, _lat.PERIODIC_BOX], ids=['wall-box', 'channel', 'periodic-box'])
@pytest.mark.parametrize('name', LATTICES)
def test_in_place_equals_two_copy(name, box, precision):
    a = _lat.run_gpu(*_lat.case(name, box, pattern='AB', precision=precision), steps=20)
    b = _lat.run_gpu(*_lat.case(name, box, pattern='AA', precision=precision), steps=20)
    wet = _lat.wet_mask(box['size'], box['walls'])
    fa, fb = _lat.merged(a, 'dist'), _lat.merged(b, 'dist')
    assert np.all(np.isfinite(fa[:, wet])) and np.array_equal(fa[:, wet], fb[:, wet])
    for what in ('rho', 'v0', 'v1', 'v2'):
        assert np.array_equal(_lat.merged(a, what)[wet], _lat.merged(b, what)[wet]), what


# ---- conservation -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', LATTICES)
def test_mass_and_momentum_are_conserved(name):
    """Periodic 32 x 8 x 8, single precision, 200 steps, no force.  Streaming moves values unchanged; a collision changes a
    node's populations by their rounding, which the bound of tests/test_gpu_fe.py lets add up over every node and step:
    (Q + 2) half-ulps of values below the node's density (at most 1.03 here) -- for the mass, and for each component of the
    momentum, which adds the same populations with signs."""
    size, steps = (32, 8, 8), 200
    grid = sym.lookup_grid(name)
    sim, cfg = _lat.case(name, dict(size=size, walls=None, force=None), pattern='AA', precision='single')
    e = np.array(grid.basis, dtype=np.float64)

    def sums(f):
        assert f.dtype == np.float32 and np.all(np.isfinite(f))
        per_dir = f.astype(np.float64).reshape(grid.Q, -1).sum(axis=1)
        return np.concatenate([[per_dir.sum()], e.T.dot(per_dir)])
    # the initial populations: the twin's (the kernels' are the same bits: every whole-step test starts from them)
    s0 = sums(tw.TwinGroup(sim, LBGeometry3D, cfg).merged('dist'))
    s1 = sums(_lat.merged(_lat.run_gpu(sim, cfg, steps), 'dist'))
    n, eps = int(np.prod(size)), float(np.finfo(np.float32).eps)
    bound = n * steps * (grid.Q + 2) * 0.5 * eps * 1.03
    drift = np.abs(s1 - s0)
    print('%s: drift of mass %.3e, of momentum %.3e %.3e %.3e (bound %.3e)' % ((name,) + tuple(drift) + (bound,)))
    assert np.all(drift <= bound)
    assert abs(s0[0] - n) < 0.05 * n and np.abs(s0[1:]).max() > 0


# ---- checkpoint -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name', LATTICES)
def test_checkpoint_round_trip(name, pattern, tmp_path):
    """13 steps and a checkpoint, restored and continued to 20 == 20 steps (13: an odd in-place iteration)."""
    sim, cfg = _lat.case(name, _lat.CHANNEL, pattern=pattern, precision='single')
    straight = _lat.run_gpu(sim, cfg, 20)
    ck = str(tmp_path / 'ck')
    _lat.run_gpu(sim, dict(cfg, checkpoint_file=ck, final_checkpoint=True), 13)
    cp = [f for f in os.listdir(str(tmp_path)) if f.startswith('ck') and f.endswith('.cpoint.npz')]
    assert len(cp) == 1
    restored = _lat.run_gpu(sim, dict(cfg, restore_from=os.path.join(str(tmp_path), cp[0][:-len('.0.cpoint.npz')])), 20)
    assert restored.runners[0]._sim.iteration == 20
    assert np.array_equal(restored.runners[0]._debug_get_dist(), straight.runners[0]._debug_get_dist(), equal_nan=True)
    assert np.array_equal(_lat.merged(restored, 'rho'), _lat.merged(straight, 'rho'))


# ---- refused again at module creation, and nothing runs D3Q19 code ----------------------------------------------------------

def _backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def _desc_kw(lattice):
    return dict(lattice=lattice, model=hipabi.SLF_BGK, precision=4, access_pattern=hipabi.SLF_AB, lat_nx=18, lat_ny=10, lat_nz=6,
                arr_nx=32, arr_ny=10, arr_nz=6, tau=1.0, visc=1.0 / 6.0, tau_phi=1.0, tau_theta=1.0, fluid_only=0, nt_type_mask=7,
                nt_misc_shift=3, type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_GHOST, hipabi.SLF_NK_FULL_BB, hipabi.SLF_NK_HALF_BB],
                fe_Gamma=0.5, fe_kappa=0.04, fe_A=0.04, fe_tau_a=1.0, fe_tau_b=1.0, bc_wall_grad_order=2,
                entropy_tolerance=1e-6, alpha_tolerance=1e-10)


MODULE_REFUSALS = [
    (dict(model=hipabi.SLF_MRT), 'model=mrt'),
    (dict(model=hipabi.SLF_ELBM), 'model=elbm'),
    (dict(regularized=1), 'regularized'),
    (dict(subgrid=hipabi.SLF_SUBGRID_LES_SMAGORINSKY, smagorinsky_const=0.1), 'subgrid'),
    (dict(incompressible=hipabi.SLF_DENSITY_ROUNDOFF), 'minimize_roundoff'),
    (dict(node_addressing=hipabi.SLF_ADDR_INDIRECT, dist_stride=4096), 'indirect'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_BINARY), 'Shan-Chen'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_SINGLE), 'Shan-Chen'),
    (dict(simtype=hipabi.SLF_SIM_FREE_ENERGY), 'free-energy'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_TERNARY), 'ternary'),
    (dict(type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_EQUILIBRIUM_VELOCITY]), 'NTHalfBBWall nodes only'),
    (dict(type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_WALL_TMS]), 'NTHalfBBWall nodes only'),
]


@pytest.mark.parametrize('over,word', MODULE_REFUSALS, ids=['%d-%s' % (i, w.split()[0]) for i, (_, w) in enumerate(MODULE_REFUSALS)])
@pytest.mark.parametrize('name', LATTICES)
def test_refused_at_module_creation(name, over, word):
    from sailfish_amd.backend_hip import HIPFatalError
    backend = _backend()
    kw = _desc_kw(sym.lookup_grid(name).slf_id)
    backend.build(hipabi.make_desc(**kw))
    kw.update(over)
    with pytest.raises(HIPFatalError, match='%s: .*%s' % (name, word)):
        backend.build(hipabi.make_desc(**kw))


def test_unknown_lattice_ids_stay_refused():
    from sailfish_amd.backend_hip import HIPFatalError
    for lattice in (4, 7):
        with pytest.raises(HIPFatalError, match='unsupported lattice'):
            _backend().build(hipabi.make_desc(**_desc_kw(lattice)))


@pytest.mark.parametrize('name', LATTICES)
def test_every_kernel_name_is_lattice_aware_or_refused(name):
    """Every name of slf::KERNEL_TABLE asked of a module of the lattice: the sweeps, the initial conditions and the
    ghost-layer kernels run the lattice's own code -- a population set in a direction D3Q19 does not have (a corner), or has
    under another number, moves the way this lattice says; the kernels that never look at a direction resolve; everything
    else refuses, the unsupported ones naming the lattice.  And the entry points outside the table refuse by name."""
    from sailfish_amd.backend_hip import HIPFatalError
    from sailfish_amd.box import BoxSim, make_box_desc
    grid = sym.lookup_grid(name)
    backend = _backend()
    names = sorted(set(re.findall(r'^  \{"(\w+)", KK_', open(os.path.join(ROOT, 'sailfish_amd', 'csrc', 'slf_bind.h')).read(), re.M)))
    assert len(names) >= 25
    module = backend.build(hipabi.make_desc(**dict(_desc_kw(grid.slf_id), access_pattern=hipabi.SLF_AA)))
    generic = {'ApplyMacroPeriodicBoundaryConditions': ([0, 0], 'Pi'), 'CollectSparseData': ([0, 0, 0, 0], 'PPPi'),
               'DistributeSparseData': ([0, 0, 0, 0], 'PPPi'), 'CollectContinuousData': ([0, 0, 2, 0, 1, 4, 32, 2], 'PPiiiiii'),
               'DistributeContinuousData': ([0, 0, 2, 0, 1, 4, 32, 2], 'PPiiiiii')}
    own = {'CollideAndPropagate': ([0] * 7 + [0], 'PPPPPPPi'), 'ComputeMacroFields': ([0] * 7 + [0], 'PPPPPPPi'),
           'SetInitialConditions': ([0] * 6, 'PPPPPP'), 'ApplyPeriodicBoundaryConditions': ([0, 0], 'Pi'),
           'ApplyPeriodicBoundaryConditionsWithSwap': ([0, 0], 'Pi')}
    for kernel in names:
        if kernel in generic or kernel in own:
            args, fmt = (generic.get(kernel) or own[kernel])
            backend.get_kernel(module, kernel, None, args, fmt, needs_iteration=kernel in ('CollideAndPropagate', 'ComputeMacroFields'))
        else:
            with pytest.raises(HIPFatalError) as info:
                backend.get_kernel(module, kernel, None, [0], 'P')
            msg = str(info.value)
            assert ('exist' in msg) or (name in msg), (kernel, msg)
            if kernel in ('CollideAndPropagateResident', 'CollectContinuousDataWithSwap', 'DistributeContinuousMacroData'):
                assert name in msg, (kernel, msg)
    with pytest.raises(HIPFatalError, match='D3Q15 / D3Q27'):
        backend.get_kernel(module, 'CollectContinuousData', None, [0, 2, 0, 1, 6, 10, 0], 'PiiiiiP')
    # outside the table
    assert not backend.supports_row_classes(module.desc)
    with pytest.raises(HIPFatalError, match='%s: row classes' % name):
        backend.classify_rows(module, 4096)
    with pytest.raises(HIPFatalError, match='force objects are not implemented on %s' % name):
        backend.force_workspace(module, 1, 10)
    lib = backend._lib
    assert lib.slf_module_set_xface_buffers(module.handle, 4096, 4096, 4096, 4096) == 3
    assert name in lib.slf_last_error().decode() and 'x-face buffers' in lib.slf_last_error().decode()
    assert lib.slf_module_set_xface_planes(module.handle, 0, 4096, 4096, 4096, 4096) == 3
    assert name in lib.slf_last_error().decode() and 'x-face planes' in lib.slf_last_error().decode()
    # the lattice's own code: one population per direction, one step each way round
    for pattern, periodic_fused in (('AB', [1, 1, 1]), ('AA', [1, 1, 1]), ('AB', [0, 0, 0]), ('AA', [0, 0, 0])):
        desc = make_box_desc(grid, (8, 6, 5), precision='single', access_pattern=pattern, periodic_fused=periodic_fused,
                             relaxation_enabled=False)
        box = BoxSim(backend, desc, periodic=(True, True, True))
        try:
            assert box.k_pair is None       # (two-copy and wrapped inside the sweep: refused by the library, naming the lattice)
            assert not (pattern == 'AB' and all(periodic_fused)) or name in box.pair_refused
            start = np.zeros((grid.Q,) + box.shape, dtype=np.float32)
            for i in range(grid.Q):
                start[i, 2, 3, 4] = 1.0 + i
            box.set_dist(start)
            if pattern == 'AB':
                box.set_dist(np.zeros_like(start), which=1)
            box.run(2, save_last=False)
            got = box.real_view(box.get_dist())
            want = np.zeros_like(got)
            for i, e in enumerate(grid.basis):
                x, y, z = (3 + 2 * e[0]) % 8, (2 + 2 * e[1]) % 6, (1 + 2 * e[2]) % 5
                want[i, z, y, x] = 1.0 + i
            assert np.array_equal(got, want), (pattern, periodic_fused)
        finally:
            box.release()


# ---- the example ------------------------------------------------------------------------------------------------------------

def test_kida_vortex_example_on_d3q15(tmp_path):
    """examples/kida_vortex.py --grid=D3Q15, 20 steps at 32^3, sampled every 10: finite, and the energy decays."""
    out = str(tmp_path / 'kida')
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'kida_vortex.py'), '--grid=D3Q15', '--max_iters=20', '--lat_nx=32',
           '--lat_ny=32', '--lat_nz=32', '--stats_every=10', '--quiet', '--output=' + out, '--every=1000', '--visc=0.01']
    done = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert done.returncode == 0, done.stderr[-3000:]
    rows = np.loadtxt(out + '_ke_ens_0.dat').reshape(-1, 3)
    print(rows)
    assert rows[:, 0].tolist() == [10.0, 20.0]
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 1:] > 0)
    assert rows[1, 1] < rows[0, 1] < 3.0 / 8.0 * 0.05 ** 2 * 1.01      # below the initial energy per node, and decaying
