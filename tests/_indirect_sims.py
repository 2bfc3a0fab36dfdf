"""Simulations and the case table of the indirect-addressing tests (tests/test_indirect_bc_oracle.py on the CPU,
tests/test_gpu_indirect.py and tests/_indirect_worker.py on the GPU); test-only.

The geometry: flow along x, walls on the two y rims, a solid block 6 nodes long and about half the channel high standing
on the lower wall (its inner nodes have no fluid neighbour: they own no slot under indirect addressing), an inlet on
hx == 0, an outlet on hx == gx - 1; z, where there is one, is periodic (`periodic_z=True` in the case's config).
The cases whose names carry `@<frame>` lay the same geometry out with the flow along y or z (make_sim's `frame`).
load_active_node_map() goes through set_active_node_map_from_wall_map(), as examples/external_geometry.py does."""
import numpy as np

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish import node_type as nt
from sailfish.lb_base import LBForcedSim
from sailfish.lb_single import LBFluidSim
from sailfish.subdomain import Subdomain2D, Subdomain3D
from sailfish.sym import D2Q9, D3Q19

U_IN = 0.03

# boundary-condition level of a node type (slf_kernels.h, Geometry::bc_level): 0 needs no boundary-condition code, 2 are the
# outflow / do-nothing / slip nodes, 1 everything else.  Written down here from the node types; not read back from the library.
LEVEL = {'NTFullBBWall': 0, 'NTHalfBBWall': 1, 'NTRegularizedVelocity': 1, 'NTZouHeVelocity': 1, 'NTEquilibriumVelocity': 1,
         'NTZouHeDensity': 1, 'NTRegularizedDensity': 1, 'NTEquilibriumDensity': 1, 'NTCopy': 2, 'NTYuOutflow': 2, 'NTSlip': 2}


def frame_axes(dim, frame):
    """(a, s, b): flow axis, sign of the flow, wall axis of a frame of tests/_faces.py; None = the x frame."""
    if frame is None:
        return 0, 1, 1
    return (frame[0], frame[1], frame[2]) if dim == 3 else (frame[0], frame[1], 1 - frame[0])


def make_sim(dim, wall='NTFullBBWall', inlet=None, outlet=None, slip=False, force=None, halfbb_solid=True, block=None,
             block_len=6, block_height=None, block_y0=1, u0=U_IN, frame=None):
    """An LBFluidSim subclass (with LBForcedSim and a body force when `force` is given).
    wall: node type of the y rims and of the block; slip: NTSlip on the y rims instead (the block keeps `wall`).
    inlet / outlet: node-type names for hx == 0 / hx == gx - 1 (velocity types get (U_IN, 0[, 0]), density types 1.0,
    outflow types nothing), or None (x periodic in the config then).
    halfbb_solid: what load_active_node_map() tells set_active_node_map_from_wall_map() about NTHalfBBWall nodes that touch
    the fluid -- True: solid, like every other wall node (the layer behind them then owns no slot); False: fluid, so that
    the layer behind them is active.
    block: x of the block's first column (default gx // 3), or 'outlet': the block ends in the column in front of the
    outlet and the outflow nodes get their orientation explicitly -- the second node upstream of an outlet node behind the
    block is then an inner node of the block, without a slot.
    block_y0: the block's first row; 1 = it stands on the lower wall.  Under slip walls it must not: the mirror image of a
    link from a slip node below the block's edge into the fluid comes out of the block, where the dense run reads the
    storage of a node that is not simulated and the sparse run has none.
    frame: a frame of tests/_faces.py -- (flow axis, sign, wall axis) in 3-D, (flow axis, sign) in 2-D -- in which all of
    the above is laid out: read "x" as the position along the flow axis counted from the upstream end, "y" as the
    position along the wall axis; the inlet velocity, `u0` and `force` (given as its size along the flow) point along
    the flow.  None = flow along +x, walls on y."""
    base = Subdomain2D if dim == 2 else Subdomain3D
    grid = D2Q9 if dim == 2 else D3Q19
    at_outlet = block == 'outlet'
    fa, fs, fb = frame_axes(dim, frame)

    def unit(axis, size):
        v = [0.0] * dim if isinstance(size, float) else [0] * dim
        v[axis] = size
        return v

    class ChannelSubdomain(base):
        def _parts(self, *h):
            """(rims, block, inlet, outlet) over the given index grids; positions outside the domain are rim.  Works in
            (position along the flow from the upstream end, position along the wall axis)."""
            g = (self.gx, self.gy) + ((self.gz,) if dim == 3 else ())
            gx, gy = g[fa], g[fb]
            hx = h[fa] if fs > 0 else gx - 1 - h[fa]
            hy = h[fb]
            rim = (hy <= 0) | (hy >= gy - 1) | (hx < 0) | (hx > gx - 1)
            x0 = (gx - 1 - block_len) if at_outlet else (gx // 3 if block is None else block)
            ht = gy // 2 if block_height is None else block_height
            blk = (hx >= x0) & (hx < x0 + block_len) & (hy >= block_y0) & (hy < block_y0 + ht) & ~rim
            free = ~rim & ~blk
            ins = free & (hx == 0) if inlet else np.zeros_like(rim)
            outs = free & (hx == gx - 1) if outlet else np.zeros_like(rim)
            inside = (hx >= 0) & (hx <= gx - 1) & (hy >= 0) & (hy <= gy - 1)
            return rim, blk, ins, outs, inside, hy, gy

        def boundary_conditions(self, *h):
            rim, blk, ins, outs, inside, hy, gy = self._parts(*h)
            rim = rim & inside      # the ghost layers stay unset
            wall_type = getattr(nt, wall)
            if slip:
                self.set_node(rim & (hy <= 0), nt.NTSlip(orientation=grid.vec_to_dir(unit(fb, 1))))
                self.set_node(rim & (hy >= gy - 1), nt.NTSlip(orientation=grid.vec_to_dir(unit(fb, -1))))
                self.set_node(blk, wall_type)
            else:
                self.set_node(rim | blk, wall_type)
            if inlet:
                self.set_node(ins, getattr(nt, inlet)(tuple(unit(fa, fs * U_IN))))
            if outlet:
                cls = getattr(nt, outlet)
                if cls.value_name == 'density':
                    self.set_node(outs, cls(1.0))
                elif at_outlet:
                    self.set_node(outs, cls(orientation=grid.vec_to_dir(unit(fa, -fs))))
                else:
                    self.set_node(outs, cls)

        def initial_conditions(self, sim, *h):
            sim.rho[:] = 1.0
            (sim.vx, sim.vy, sim.vz if dim == 3 else None)[fa][:] = fs * u0

        def solid_map(self, *h):
            rim, blk = self._parts(*h)[:2]
            return rim | blk

        def load_active_node_map(self, *h):
            solid = self.solid_map(*h)
            if wall == 'NTHalfBBWall' and not halfbb_solid:
                # half-way bounce-back nodes next to the fluid are wet nodes: count them as fluid, so that the nodes their
                # even in-place step stores into (the layer behind them) own a slot
                near = np.zeros_like(solid)
                for off in self._neighbour_offsets():
                    if any(off):
                        near |= np.roll(~solid, shift=tuple(-o for o in off), axis=tuple(range(solid.ndim)))
                solid = solid & ~near
            self.set_active_node_map_from_wall_map(solid)

    bases = (LBFluidSim, LBForcedSim) if force is not None else (LBFluidSim,)

    class ChannelSim(*bases):
        subdomain = ChannelSubdomain

        def __init__(self, config):
            super(ChannelSim, self).__init__(config)
            if force is not None:
                self.add_body_force(tuple(force) if frame is None else tuple(unit(fa, fs * float(force[0]))))

    return ChannelSim


def cavity_sim(dim):
    """A closed box of full-way bounce-back walls with the block inside and a regularized-velocity lid on the upper y rim
    (the cavity of tests/test_gpu_reg_les.py, with storage for the active nodes only)."""
    base = Subdomain2D if dim == 2 else Subdomain3D

    class CavitySubdomain(base):
        def _solid(self, hx, hy):
            outside = (hx <= 0) | (hx >= self.gx - 1) | (hy <= 0)
            x0 = self.gx // 3
            return outside | ((hx >= x0) & (hx < x0 + 6) & (hy <= self.gy // 2))

        def boundary_conditions(self, hx, hy, *hz):
            solid = self._solid(hx, hy)
            self.set_node(solid & (hx >= 0) & (hx <= self.gx - 1) & (hy >= 0), nt.NTFullBBWall)
            self.set_node(~solid & (hy == self.gy - 1), nt.NTRegularizedVelocity((0.05,) + (0.0,) * (dim - 1)))

        def initial_conditions(self, sim, hx, hy, *hz):
            sim.rho[:] = 1.0

        def load_active_node_map(self, hx, hy, *hz):
            self.set_active_node_map_from_wall_map(self._solid(hx, hy) | (hy > self.gy - 1))

    class CavitySim(LBFluidSim):
        subdomain = CavitySubdomain

    return CavitySim


# ---- the case table -------------------------------------------------------------------------------------------------------
SIZE = {2: dict(lat_nx=40, lat_ny=14), 3: dict(lat_nx=40, lat_ny=12, lat_nz=6, periodic_z=True)}
GRID = {2: 'D2Q9', 3: 'D3Q19'}
# the frames (tests/_faces.py) beyond the x frame that the table adds: flow along y / z, both senses, walls on each other axis
OTHER_FRAMES = {2: [(1, 1), (1, -1)], 3: [(a, s, b) for a in (1, 2) for s in (1, -1) for b in range(3) if b != a]}
ALL_PM = [(p, m) for p in ('single', 'double') for m in ('bgk', 'mrt')]


def _cfg(dim, precision, model, pattern, **kw):
    return dict(SIZE[dim], grid=GRID[dim], visc=0.05, precision=precision, model=model, access_pattern=pattern,
                node_addressing='indirect', **kw)


def _steps(pattern):
    """In place: an even and an odd number of steps, so that both step kinds finish a run; two-copy: 20."""
    return (20, 21) if pattern == 'AA' else (20,)


def _build_cases():
    """name -> dict(sim: make_sim keywords | ('cavity', dim) | (example module, class), dim, cfg, steps, level, vmin,
    dense: compare with the dense run on the CPU)."""
    cases = {}

    def add(name, sim, dim, cfg, pattern, level, vmin=1e-3, dense=True, steps=None):
        for n in (steps or _steps(pattern)):
            cases['%s-%d' % (name, n)] = dict(sim=sim, dim=dim, cfg=cfg, steps=n, level=level, vmin=vmin, dense=dense)

    def tag(dim, precision, model, pattern):
        return 'd%d-%s-%s-%s' % (dim, 'f32' if precision == 'single' else 'f64', model, pattern)

    for dim in (2, 3):
        # level 1, velocity in / density out
        types = dict(wall='NTFullBBWall', inlet='NTRegularizedVelocity', outlet='NTZouHeDensity')
        for precision, model in ALL_PM:
            for pattern in ('AA', 'AB'):
                add('regvel_zhrho-' + tag(dim, precision, model, pattern), dict(dim=dim, **types), dim,
                    _cfg(dim, precision, model, pattern), pattern, 1)
        # level 1, other kinds (two-copy)
        types = dict(wall='NTHalfBBWall', inlet='NTEquilibriumVelocity', outlet='NTRegularizedDensity')
        for precision, model in (('double', 'bgk'), ('single', 'mrt')):
            add('halfbb_eqvel_regrho-' + tag(dim, precision, model, 'AB'), dict(dim=dim, **types), dim,
                _cfg(dim, precision, model, 'AB'), 'AB', 1)
        # level 1, half-way walls in place, the layer behind the walls active
        types = dict(wall='NTHalfBBWall', inlet='NTZouHeVelocity', outlet='NTEquilibriumDensity', halfbb_solid=False)
        for precision, model in ALL_PM:
            add('halfbb_inplace-' + tag(dim, precision, model, 'AA'), dict(dim=dim, **types), dim,
                _cfg(dim, precision, model, 'AA'), 'AA', 1)
        # level 2, outflow (two-copy only, as in the reference)
        for short, types in (('copy', dict(wall='NTFullBBWall', inlet='NTRegularizedVelocity', outlet='NTCopy')),
                             ('yu', dict(wall='NTHalfBBWall', inlet='NTZouHeVelocity', outlet='NTYuOutflow'))):
            for precision, model in ALL_PM:
                add('%s-%s' % (short, tag(dim, precision, model, 'AB')), dict(dim=dim, **types), dim,
                    _cfg(dim, precision, model, 'AB'), 'AB', 2)
            # the block in front of the outlet: upstream neighbours without a slot; against the sparse oracle only (the dense
            # run reads a wall node's storage there)
            add('%s_guard-%s' % (short, tag(dim, 'single', 'bgk', 'AB')), dict(dim=dim, block='outlet', **types), dim,
                _cfg(dim, 'single', 'bgk', 'AB'), 'AB', 2, dense=False)
        # level 2, slip walls, body force, x periodic
        force = (1e-5,) + (0.0,) * (dim - 1)
        for precision in ('single', 'double'):
            for pattern in ('AA', 'AB'):
                add('slip-' + tag(dim, precision, 'bgk', pattern), dict(dim=dim, slip=True, force=force, block_y0=3), dim,
                    _cfg(dim, precision, 'bgk', pattern, periodic_x=True, force_implementation='guo'), pattern, 2)
        # (beyond the slip row above: MRT in place, the level-2 instantiations no other case reaches)
        for precision in ('single', 'double'):
            add('slip-' + tag(dim, precision, 'mrt', 'AA'), dict(dim=dim, slip=True, force=force, block_y0=3), dim,
                _cfg(dim, precision, 'mrt', 'AA', periodic_x=True, force_implementation='guo'), 'AA', 2)
        # --minimize_roundoff: forced channels between full-way / half-way walls (in place: the layer behind the half-way
        # walls active)
        for wall in ('NTFullBBWall', 'NTHalfBBWall'):
            for precision in ('single', 'double'):
                for pattern in ('AA', 'AB'):
                    add('roundoff_%s-%s' % (wall[2:8].lower(), tag(dim, precision, 'bgk', pattern)),
                        dict(dim=dim, wall=wall, force=force, halfbb_solid=False), dim,
                        _cfg(dim, precision, 'bgk', pattern, periodic_x=True, force_implementation='guo',
                             minimize_roundoff=True), pattern, LEVEL[wall])
        # --regularized, --subgrid=les-smagorinsky: a cavity with the block
        for opt, kw in (('reg', dict(regularized=True)), ('les', dict(subgrid='les-smagorinsky', smagorinsky_const=0.1))):
            for precision in ('single', 'double'):
                for pattern in ('AA', 'AB'):
                    add('%s-%s' % (opt, tag(dim, precision, 'bgk', pattern)), ('cavity', dim), dim,
                        dict(_cfg(dim, precision, 'bgk', pattern, **kw), visc=0.004), pattern, 1)
        # region launches: two subdomains, cut along y (2-D) / z (3-D)
        types = dict(wall='NTFullBBWall', inlet='NTRegularizedVelocity', outlet='NTZouHeDensity')
        for pattern in ('AA', 'AB'):
            add('regions-' + tag(dim, 'double', 'bgk', pattern), dict(dim=dim, **types), dim,
                _cfg(dim, 'double', 'bgk', pattern, subdomains=2, conn_axis='y' if dim == 2 else 'z'), pattern, 1)
    # other frames: the flow along y and along z, both senses, the walls on each remaining axis -- the outflow look-ups
    # one / two nodes upstream, the in-place half-way store and the slip reflection then cross rows and planes
    for dim in (2, 3):
        for frame in OTHER_FRAMES[dim]:
            fa, fs, fb = frame_axes(dim, frame)
            ftag = '%s%s' % ('+' if fs > 0 else '-', 'xyz'[fa]) + ('_walls_%s' % 'xyz'[fb] if dim == 3 else '')

            def ftagged(precision, model, pattern):
                return '%s@%s' % (tag(dim, precision, model, pattern), ftag)

            def fcfg(precision, model, pattern, periodic_flow=False, **kw):
                ext = [0] * dim
                ext[fa], ext[fb] = SIZE[dim]['lat_nx'], SIZE[dim]['lat_ny']
                cfg = dict(grid=GRID[dim], visc=0.05, precision=precision, model=model, access_pattern=pattern,
                           node_addressing='indirect', **kw)
                if dim == 3:
                    fc = 3 - fa - fb
                    ext[fc] = SIZE[dim]['lat_nz']
                    cfg['periodic_' + 'xyz'[fc]] = True
                if periodic_flow:
                    cfg['periodic_' + 'xyz'[fa]] = True
                cfg.update(('lat_n' + 'xyz'[k], ext[k]) for k in range(dim))
                return cfg

            types = dict(wall='NTFullBBWall', inlet='NTRegularizedVelocity', outlet='NTZouHeDensity', frame=frame)
            for precision in ('single', 'double'):
                add('regvel_zhrho-' + ftagged(precision, 'bgk', 'AA'), dict(dim=dim, **types), dim,
                    fcfg(precision, 'bgk', 'AA'), 'AA', 1)
            types = dict(wall='NTFullBBWall', inlet='NTRegularizedVelocity', outlet='NTCopy', frame=frame)
            add('copy-' + ftagged('single', 'bgk', 'AB'), dict(dim=dim, **types), dim, fcfg('single', 'bgk', 'AB'), 'AB', 2)
            types = dict(wall='NTHalfBBWall', inlet='NTZouHeVelocity', outlet='NTYuOutflow', frame=frame)
            add('yu_guard-' + ftagged('single', 'bgk', 'AB'), dict(dim=dim, block='outlet', **types), dim,
                fcfg('single', 'bgk', 'AB'), 'AB', 2, dense=False)
            types = dict(wall='NTHalfBBWall', inlet='NTZouHeVelocity', outlet='NTEquilibriumDensity', halfbb_solid=False,
                         frame=frame)
            add('halfbb_inplace-' + ftagged('single', 'bgk', 'AA'), dict(dim=dim, **types), dim,
                fcfg('single', 'bgk', 'AA'), 'AA', 1)
            add('slip-' + ftagged('single', 'mrt', 'AA'), dict(dim=dim, slip=True, force=(1e-5,), block_y0=3, frame=frame),
                dim, fcfg('single', 'mrt', 'AA', periodic_flow=True, force_implementation='guo'), 'AA', 2)
    # level 0 in double: the two examples the single-precision tests use
    for model in ('bgk', 'mrt'):
        for pattern in ('AA', 'AB'):
            add('extgeo-' + tag(3, 'double', model, pattern), ('external_geometry', 'ExternalSimulation'), 3,
                dict(lat_nx=48, lat_ny=21, lat_nz=21, visc=0.05, periodic_x=True, grid='D3Q19', node_addressing='indirect',
                     precision='double', model=model, access_pattern=pattern), pattern, 0, vmin=1e-6)
            add('cylinder-' + tag(2, 'double', model, pattern), ('cylinder', 'CylinderSimulation'), 2,
                dict(lat_nx=60, lat_ny=36, visc=0.1, vertical=False, force_implementation='guo', node_addressing='indirect',
                     precision='double', model=model, access_pattern=pattern), pattern, 0, vmin=1e-6)
    # (D2Q9 f32 MRT at level 0: the one combination of lattice, precision and model the f32 tests of tests/test_gpu_runner.py
    # leave out)
    for pattern in ('AA', 'AB'):
        add('cylinder-' + tag(2, 'single', 'mrt', pattern), ('cylinder', 'CylinderSimulation'), 2,
            dict(lat_nx=60, lat_ny=36, visc=0.1, vertical=False, force_implementation='guo', node_addressing='indirect',
                 precision='single', model='mrt', access_pattern=pattern), pattern, 0, vmin=1e-6)
    # level 0 and 1, f32 BGK D3Q19 in place: the odd step of both runs the level-1 kernel (launch_slot_sweep)
    add('skip0_level0-' + tag(3, 'single', 'bgk', 'AA'), dict(dim=3, wall='NTFullBBWall', force=(1e-5, 0.0, 0.0)), 3,
        _cfg(3, 'single', 'bgk', 'AA', periodic_x=True, force_implementation='guo'), 'AA', 0)
    add('skip0_level1-' + tag(3, 'single', 'bgk', 'AA'),
        dict(dim=3, wall='NTFullBBWall', inlet='NTRegularizedVelocity', outlet='NTZouHeDensity'), 3,
        _cfg(3, 'single', 'bgk', 'AA'), 'AA', 1)
    # slot-count edges (2-D, f32 BGK, in place); the counts are asserted in tests/test_indirect_bc_oracle.py
    types = dict(dim=2, wall='NTFullBBWall', inlet='NTRegularizedVelocity', outlet='NTZouHeDensity')
    for name, size, extra in (('under256', dict(lat_nx=16, lat_ny=10), dict(block=5, block_len=3)),
                              ('multiple256', dict(lat_nx=41, lat_ny=14), dict(block_len=12, block_height=9)),
                              ('padded', dict(lat_nx=40, lat_ny=14), dict(block_len=7))):
        add('slots_' + name, dict(types, **extra), 2, dict(_cfg(2, 'single', 'bgk', 'AA'), **size), 'AA', 1)
    return cases


CASES = _build_cases()
# slot-count edges: (active nodes) -> what must hold
SLOT_EDGES = {'slots_under256': lambda n, stride: n < 256,
              'slots_multiple256': lambda n, stride: n % 256 == 0 and n > 0,
              'slots_padded': lambda n, stride: stride > n + 1}


def sim_class(case):
    sim = case['sim']
    if isinstance(sim, dict):
        return make_sim(**sim)
    if sim[0] == 'cavity':
        return cavity_sim(sim[1])
    from tests import _host
    return _host.load_sim_class(*sim)


def fluid_mask(runners, gshape):
    """The plain fluid nodes of the global domain (visualization_map() == 0)."""
    wet = np.zeros(gshape, dtype=bool)
    for r in runners:
        sp = r._spec
        sl = tuple(slice(o, o + n) for o, n in zip(reversed(sp.location), reversed(sp.size)))
        wet[sl] = r._subdomain.visualization_map() == 0
    return wet
