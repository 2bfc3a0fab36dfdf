"""Boundary nodes on every face, through the dense sweep kernels: the channels of tests/_faces.py with their flow along
any axis, in either sense, and their walls on any other axis, BoxSim against the CPU oracle bit for bit.  The oracle is
frame-invariant (tests/test_oracle_faces.py: all frames agree within 1e-12 in double precision), so agreement with it in
a frame means that the kernel is right there.

Shapes: 70 nodes along x whatever the role of x (two waves, the last partly idle), 24 along the flow, 9 between the
walls, 6 along the periodic axis wherever that axis is not x; 30 and 31 steps, so that both kinds of in-place step end
a run.  f32: rho / u within 1e-6 (relative to the speed scale 0.03), f64: within 1e-12, populations bit-identical in
both precisions."""
import numpy as np
import pytest

from sailfish_amd import sym
from tests import _faces as F
from tests import _geometry as geo
from tests._pair import run_pair

pytestmark = pytest.mark.gpu

STEPS = (30, 31)


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def _size(grid, frame):
    return F.size_of(frame, 24, 9, 6 if grid.dim == 3 else None, nx=70)


def _bc_rows_of(desc, nmap):
    """Real rows (y, z) with a node that is neither fluid nor excluded nor a full-way wall: what
    slf_module_classify_rows lists (slf_row.hip: classify_rows_kernel)."""
    real = nmap[1:desc.lat_nz - 1, 1:desc.lat_ny - 1, 1:desc.lat_nx - 1] & ((1 << geo.NT_BITS[0]) - 1)
    plain = np.isin(real, (geo.T_FLUID, geo.T_GHOST, geo.T_UNUSED, geo.T_FULLBB))
    return int(np.count_nonzero(~plain.all(axis=2)))


def _check(backend, grid, frame, case, look=None):
    size = _size(grid, frame)
    assert size[0] == 70
    periodic, node_map_fn, init, kw = F.setup(grid, frame, case, size)
    tol = 1e-12 if case[3] == 'double' else 1e-6
    for steps in STEPS:
        r, g, o = run_pair(backend, grid, size, steps, periodic, node_map_fn=node_map_fn, u_scale=F.U, init=init,
                           sims=True, **kw)
        print(F.frame_id(frame), F.case_id(case), steps, r)
        assert r['rho_err'] < tol and r['v_err'] < tol, (steps, r)
        assert r['dist_exact'], (steps, r)
        # the boundary did something: the speed along the flow is not uniform over the layer it acts on
        g_rho, g_v = g.fetch_fields()
        fields = F.to_x_frame((g.real_view(g_rho), [g.real_view(c) for c in g_v[:grid.dim]]), frame)
        layer = F.outlet_layer(fields[1][0], frame, case[0])
        fin = np.isfinite(layer)
        assert fin.any() and np.ptp(layer[fin]) > 0
        if grid.dim == 3 and g.row_classes is not None:
            # the rows listed for the boundary-condition instantiation (slf_row.hip: launch_row5)
            rc = g.row_classes
            assert rc['rows'] == size[1] * size[2] and rc['bc_rows'] == _bc_rows_of(g.desc, node_map_fn(g.desc)), rc
        if look:
            look(g, o)
        g.release()


@pytest.mark.parametrize('case', F.CASES_3D, ids=F.case_id)
@pytest.mark.parametrize('frame', F.FRAMES_3D, ids=F.frame_id)
def test_d3q19_every_frame(backend, frame, case):
    """Every case compares the number of rows listed for the boundary-condition instantiation with a count on the host
    (_check).  The extremes by name, for the open channels (full-way walls): a row that lies wholly in a full-way wall
    holds no boundary-condition node, so an x-flow frame lists every row but those -- the inlet column is in all others
    (every row without exception: test_d3q19_open_channel_between_slip_walls) -- and a z-flow frame lists exactly the
    rows of its two face planes (with the walls on y: but the two wall rows of each)."""
    a, s, b, c = F.axes(frame)
    nx, ny, nz = _size(sym.D3Q19, frame)

    def look(g, o):
        rc = g.row_classes
        if case[0] not in F.OPEN:
            return
        if a == 0:
            assert rc['bc_rows'] == rc['rows'] - 2 * (nz if b == 1 else ny), rc
        elif a == 2:
            assert rc['bc_rows'] == 2 * (ny if b == 0 else ny - 2), rc
    _check(backend, sym.D3Q19, frame, case, look)


@pytest.mark.parametrize('case', F.CASES_2D, ids=F.case_id)
@pytest.mark.parametrize('frame', F.FRAMES_2D, ids=F.frame_id)
def test_d2q9_every_frame(backend, frame, case):
    """The per-node kernel."""
    _check(backend, sym.D2Q9, frame, case)


@pytest.mark.parametrize('case', [c for c in F.CASES_3D if c[0] in ('zh', 'dn')], ids=F.case_id)
@pytest.mark.parametrize('frame', F.FRAMES_3D, ids=F.frame_id)
def test_d3q19_every_frame_without_row_classes(backend, frame, case, monkeypatch):
    """SLF_ROW_CLASSES=0: every row through the module's full instantiation, in one launch."""
    monkeypatch.setenv('SLF_ROW_CLASSES', '0')

    def look(g, o):
        assert g.row_classes is None
    _check(backend, sym.D3Q19, frame, case, look)


@pytest.mark.parametrize('case', F.EXTRA_3D, ids=F.case_id)
@pytest.mark.parametrize('frame', F.FRAMES_3D, ids=F.frame_id)
def test_d3q19_open_channel_between_slip_walls(backend, frame, case):
    """With slip walls every row of an x-flow frame holds a boundary-condition node, and so does every row when the walls
    are on x: n_bc_rows == n_rows, and the level-0 launch is skipped (slf_row.hip: launch_row5)."""
    def look(g, o):
        rc = g.row_classes
        if frame[0] == 0 or frame[2] == 0:
            assert rc['bc_rows'] == rc['rows'], rc
        else:
            assert 0 < rc['bc_rows'] < rc['rows'], rc
    _check(backend, sym.D3Q19, frame, case, look)


# ---- through the controller: direct addressing, one subdomain and two ---------------------------------------------------
RUNNER_CASES = {
    # flow along y between slip walls on x: the first / last column is dry, so in place the runner tells the sweeps that
    # nothing reads the x ghost columns (SubdomainRunner._init_compute: set_x_ghost_unused) -- and slip_reflect swaps
    # exactly the populations that the whole-row kernels shift along x
    'slip_on_x-AA': dict(frame=(1, 1, 0), sim=dict(walls='slip'), pattern='AA', steps=(40, 41), x_ghost_unused=True),
    'slip_on_x-AB': dict(frame=(1, 1, 0), sim=dict(walls='slip'), pattern='AB', steps=(40,), x_ghost_unused=True),
    # flow along -z, walls on x, do-nothing outlet in place: its even step stores into the ghost plane z = 0, which with
    # two subdomains cut across the flow belongs to the second one alone
    'dn_-z-AA': dict(frame=(2, -1, 0), sim=dict(), pattern='AA', steps=(40, 41)),
    'dn_-z-AA-z2': dict(frame=(2, -1, 0), sim=dict(), pattern='AA', steps=(40, 41), cfg=dict(subdomains=2, conn_axis='z')),
    # flow along +y, Yu outflow (two-copy), two subdomains cut along x: each holds one wall, the outlet row crosses the seam
    # (the upstream neighbours of the outlet nodes next to the seam hold populations that came from the other subdomain: they
    # must be in the arrays, so such modules take no x-face buffers -- sailfish_amd/xface.py: supported())
    'yu_+y-AB-x2': dict(frame=(1, 1, 0), sim=dict(inlet='NTZouHeVelocity', outlet='NTYuOutflow'), pattern='AB', steps=(40,),
                        cfg=dict(subdomains=2, conn_axis='x'), xface=False),
    'copy_-z-AB-x2': dict(frame=(2, -1, 0), sim=dict(inlet='NTZouHeVelocity', outlet='NTCopy'), pattern='AB', steps=(40,),
                          cfg=dict(subdomains=2, conn_axis='x'), xface=False),
    # the same cut with outlets that read nothing upstream: through the x-face buffers
    'dn_+y-AA-x2': dict(frame=(1, 1, 0), sim=dict(), pattern='AA', steps=(40, 41), cfg=dict(subdomains=2, conn_axis='x'),
                        xface=True),
    'zhrho_+y-AB-x2': dict(frame=(1, 1, 0), sim=dict(inlet='NTZouHeVelocity', outlet='NTZouHeDensity'), pattern='AB',
                           steps=(40,), cfg=dict(subdomains=2, conn_axis='x'), xface=True),
}


@pytest.mark.parametrize('case', sorted(RUNNER_CASES))
def test_open_ducts_through_the_runner(case):
    """set_node() -> orientation detection -> encoder -> type table -> kernels in frames other than x, against the oracle
    twin, bit for bit."""
    from tests import _open_sims
    from tests.test_gpu_runner import check_against_oracle
    c = RUNNER_CASES[case]
    size = F.size_of(c['frame'], 24, 9, 6, nx=70)
    sim = _open_sims.framed_sim(3, c['frame'], **c['sim'])
    cfg = dict(zip(('lat_nx', 'lat_ny', 'lat_nz'), size), visc=F.VISC, access_pattern=c['pattern'], **c.get('cfg', {}))
    cfg.update(sim.periodic_cfg)
    for steps in c['steps']:
        ctrl, exact = check_against_oracle(sim, None, 3, cfg, steps, 0.04)
        assert exact, steps
        assert len(ctrl.runners) == cfg.get('subdomains', 1)
        for r in ctrl.runners:
            assert r._sim.iteration == steps
            if 'xface' in c:
                assert (r._xface is not None) == c['xface']
            if c.get('x_ghost_unused'):
                assert not r._subdomain.fluid_map(wet=True)[..., 0].any() and not r._subdomain.fluid_map(wet=True)[..., -1].any()
            r.release()


RESIDENT_CASES = {
    'poiseuille_vertical_pressure': ('poiseuille', 'PoiseuilleSim',
                                     dict(lat_nx=30, lat_ny=36, visc=0.05, horizontal=False, drive='pressure', wall='fullbb'),
                                     {'AA': True, 'AB': True}),
    'slip_channel_along_y': (lambda: _framed_2d(walls='slip', inlet=None, outlet=None, force=1e-5, u0=0.0), None,
                             dict(lat_nx=30, lat_ny=36, visc=0.05, force_implementation='guo'), {'AA': True, 'AB': True}),
    # NTDoNothing: fluid nodes in the two-copy pattern (taken); in place the nodes store into memory from their node code
    # -- the ghost ROW behind them here --, the library refuses the kernel and the runner steps
    'do_nothing_along_y': (lambda: _framed_2d(u0=0.05), None, dict(lat_nx=36, lat_ny=48, visc=0.05),
                           {'AA': False, 'AB': True}),
}


def _framed_2d(**kw):
    from tests import _open_sims
    return _open_sims.framed_sim(2, (1, 1), **kw)


@pytest.mark.parametrize('case', sorted(RESIDENT_CASES))
@pytest.mark.parametrize('pattern', ['AA', 'AB'])
def test_resident_steps_equal_plain_stepping_along_y(case, pattern, monkeypatch):
    """Several steps per launch (slf_resident.hip) with the flow along y: the arrays are, slot for slot, what one launch per
    step leaves behind (as tests/test_gpu_resident.py: test_resident_steps_equal_plain_stepping has it for x)."""
    from tests.test_gpu_resident import _state
    from tests.test_gpu_runner import run_gpu
    monkeypatch.setenv('SLF_RESIDENT_FORCE', '1')
    module, sim, cfg, taken = RESIDENT_CASES[case]
    if sim is None:
        module = module()
        cfg = dict(cfg, **module.periodic_cfg)
    res = {}
    for resident in (True, False):
        ctrl = run_gpu(module, sim, 2, dict(cfg, access_pattern=pattern), 75,
                       extra=dict(hip_resident=resident, hip_graphs=resident, every=75))
        r = ctrl.runners[0]
        assert r._sim.iteration == 75
        res[resident] = _state(r)
        assert bool(r._resident) == (resident and taken[pattern])
    for a, b in zip(res[True], res[False]):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    assert np.nanmax(np.abs(res[True][-1])) > 1e-4          # the flow along y moves
