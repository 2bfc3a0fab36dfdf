"""Channel geometries in any frame (test-only helper): the node maps of tests/_geometry.py have their flow along +x
and their walls on y; here the same channels are built with the flow along any axis, in either sense, and the walls
on any other axis -- every one a mirror image / rotation of the x frame, so that the oracle's results in all frames are
the same flow (tests/test_oracle_faces.py) and a kernel that agrees with the oracle in a frame is right there.

Frame: 3-D (a, s, b) = flow axis, sign of the flow, wall axis; the third axis c is periodic.  2-D (a, s): walls on the
other axis.  Axes are 0, 1, 2 = x, y, z.  The x frame is (0, +1, 1) / (0, +1).  Orientation codes come from
grid.vec_to_dir, never from a table typed in here.

A geometry is laid out in the x frame on the real nodes (arrays indexed [c, b, a]) as node types, parameter slots and
inward normals, then carried to the frame and encoded like tests/_geometry.py does."""
import numpy as np

from sailfish_amd import sym
from tests import _geometry as geo

U = 0.03                     # inlet speed and initial speed along the flow axis
VISC = 0.05
FORCE, FORCE_C = 1e-5, 2e-6  # body force of the forced duct along the flow / along the periodic axis

FRAMES_3D = [(a, s, b) for a in range(3) for s in (1, -1) for b in range(3) if b != a]
FRAMES_2D = [(a, s) for a in range(2) for s in (1, -1)]
X_FRAME = {2: (0, 1), 3: (0, 1, 1)}


def frames(dim):
    return FRAMES_3D if dim == 3 else FRAMES_2D


def frame_id(frame):
    return '%s%s' % ('+' if frame[1] > 0 else '-', 'xyz'[frame[0]]) + ('_walls_%s' % 'xyz'[frame[2]] if len(frame) == 3 else '')


def axes(frame):
    """(a, s, b, c); c is None in 2-D."""
    if len(frame) == 3:
        a, s, b = frame
        return a, s, b, 3 - a - b
    a, s = frame
    return a, s, 1 - a, None


def size_of(frame, along, across, third=None, nx=None):
    """(nx, ny[, nz]) of a box with `along` nodes on the flow axis, `across` between the walls and `third` on the
    periodic axis; nx: the extent along x whatever the role of x."""
    a, s, b, c = axes(frame)
    size = [0] * (2 if c is None else 3)
    size[a], size[b] = along, across
    if c is not None:
        size[c] = third
    if nx is not None:
        size[0] = nx
    return tuple(size)


def _perm(frame):
    """Array axes of the frame ([z,] y, x) as positions in the x-frame layout ([c,] b, a)."""
    a, s, b, c = axes(frame)
    dim = 2 if c is None else 3
    pos = {a: dim - 1, b: dim - 2}
    if c is not None:
        pos[c] = 0
    return [pos[dim - 1 - j] for j in range(dim)]


def from_x_frame(arr, frame):
    """An array laid out in the x frame ([c,] b, a; upstream end first) -> the frame's ([z,] y, x)."""
    if frame[1] < 0:
        arr = arr[..., ::-1]
    return np.ascontiguousarray(arr.transpose(_perm(frame)))


def vec_from_x_frame(n, frame):
    a, s, b, c = axes(frame)
    out = [0] * (2 if c is None else 3)
    out[a], out[b] = s * n[0], n[1]
    if c is not None:
        out[c] = n[2]
    return out


def scalar_to_x_frame(arr, frame):
    """A scalar field (or a mask) on the real nodes of a frame -> the x frame."""
    arr = np.asarray(arr).transpose(list(np.argsort(_perm(frame))))
    return arr[..., ::-1] if frame[1] < 0 else arr


def to_x_frame(fields, frame):
    """(rho, [v...]) on the real nodes of a frame -> the same in the x frame: transposed, flipped along the flow axis
    for s < 0, velocity components reordered and signed."""
    a, s, b, c = axes(frame)
    rho, v = fields
    comps = [s * scalar_to_x_frame(v[a], frame), scalar_to_x_frame(v[b], frame)]
    if c is not None:
        comps.append(scalar_to_x_frame(v[c], frame))
    return scalar_to_x_frame(rho, frame), comps


class _Layout(object):
    """Node types, parameter slots and inward normals on the real nodes, in the x frame."""

    def __init__(self, desc, frame):
        a, s, b, c = axes(frame)
        self.dim = 2 if c is None else 3
        real = [desc.lat_nx - 2, desc.lat_ny - 2, desc.lat_nz - 2]
        self.shape = tuple(([real[c]] if c is not None else []) + [real[b], real[a]])
        self.typ = np.full(self.shape, geo.T_FLUID, dtype=np.int64)
        self.param = np.zeros(self.shape, dtype=np.int64)
        self.normal = np.zeros(self.shape, dtype=np.int64)      # index into self.normals, 0 = none
        self.normals = [None]

    def put(self, where, typ, normal=None, param=0):
        self.typ[where] = typ
        self.param[where] = param
        if normal is None:
            self.normal[where] = 0
        else:
            n = tuple(normal) + (0,) * (3 - len(normal))
            if n not in self.normals:
                self.normals.append(n)
            self.normal[where] = self.normals.index(n)

    def node_map(self, grid, desc, frame):
        orient = np.zeros(len(self.normals), dtype=np.int64)
        for k, n in enumerate(self.normals):
            if n is not None:
                orient[k] = grid.vec_to_dir(vec_from_x_frame(n[:self.dim] if self.dim == 2 else n, frame))
        code = (orient[self.normal] << geo.ORIENT_SHIFT) | (self.param << geo.NT_BITS[0]) | self.typ
        code = from_x_frame(code, frame).astype(np.uint32)
        m = geo.empty_map(desc)
        if self.dim == 3:
            m[1:desc.lat_nz - 1, 1:desc.lat_ny - 1, 1:desc.lat_nx - 1] = code
        else:
            m[0, 1:desc.lat_ny - 1, 1:desc.lat_nx - 1] = code
        return m


def _walls(lay, walls, t_slip=geo.T_SLIP):
    low, high = (Ellipsis, 0, slice(None)), (Ellipsis, -1, slice(None))
    if walls == 'slip':
        lay.put(low, t_slip, (0, 1, 0)[:lay.dim])
        lay.put(high, t_slip, (0, -1, 0)[:lay.dim])
    elif walls == 'fullbb':
        lay.put(low, geo.T_FULLBB)
        lay.put(high, geo.T_FULLBB)
    elif walls == 'halfbb-orientation':
        lay.put(low, geo.T_HALFBB, (0, 1, 0)[:lay.dim])
        lay.put(high, geo.T_HALFBB, (0, -1, 0)[:lay.dim])
    elif walls == 'halfbb-tags':        # the tags are filled in on the finished map: fill_link_tags
        lay.put(low, geo.T_HALFBB)
        lay.put(high, geo.T_HALFBB)
    else:
        raise ValueError(walls)


def open_channel(desc, frame, t_in, t_out, walls='fullbb', grid=None, out_normal=(-1, 0, 0)):
    """Inlet t_in on the upstream face of the flow axis (parameter slot 0: the velocity), outlet t_out on the downstream
    face (slot dim: the density), both with their inward normals; walls ('fullbb' / 'slip') on both faces of the wall
    axis, edges included (the edge nodes of slip walls are full-way ones); the third axis periodic.  out_normal: the outlet's normal in the x frame, for tests that
    want a wrong one."""
    lay = _Layout(desc, frame)
    grid = grid or (sym.D2Q9 if lay.dim == 2 else sym.D3Q19)
    lay.put((Ellipsis, slice(None), 0), t_in, (1, 0, 0)[:lay.dim], 0)
    lay.put((Ellipsis, slice(None), -1), t_out, tuple(out_normal)[:lay.dim], lay.dim)
    _walls(lay, walls)
    if walls == 'slip':
        # a slip node exchanges populations with its neighbours along the wall: at the two ends of the channel those
        # would be ghost nodes, so the wall ends in full-way nodes there
        for end in (0, -1):
            lay.put((Ellipsis, [0, -1], end), geo.T_FULLBB)
    return lay.node_map(grid, desc, frame)


def forced_duct(desc, frame, walls='slip', grid=None):
    """Periodic along the flow axis and the third one, walls ('slip' / 'halfbb-tags' / 'halfbb-orientation') on the wall
    axis, one full-way bounce-back block that touches no wall -- one fluid layer lies between it and the low wall, which
    therefore sees a disturbed flow however far apart the walls are --, a third of the way down from the upstream end
    (and not across the whole third axis).  The body force is force_of(frame)."""
    lay = _Layout(desc, frame)
    grid = grid or (sym.D2Q9 if lay.dim == 2 else sym.D3Q19)
    _walls(lay, walls)
    nb, na = lay.shape[-2], lay.shape[-1]
    block = (slice(2, 4), slice(na // 3, na // 3 + 3))
    lay.put(((slice(1, 3),) if lay.dim == 3 else ()) + block, geo.T_FULLBB)
    m = lay.node_map(grid, desc, frame)
    if walls == 'halfbb-tags':
        a, s, b, c = axes(frame)
        fill_link_tags(grid, desc, m, [a] + ([c] if c is not None else []))
    return m


def fill_link_tags(grid, desc, m, periodic_axes):
    """Half-way wall nodes get their link tags (geo.link_tags), with the periodic images of `periodic_axes` seen through
    the ghost layers, as geo.channel_2d_halfbb does for x."""
    mm = m.copy()
    lat = [desc.lat_nx, desc.lat_ny, desc.lat_nz]
    for k in periodic_axes:
        ax = 2 - k                                   # array axis of m[z, y, x]
        sl = [slice(None)] * 3
        lo, hi, first, last = list(sl), list(sl), list(sl), list(sl)
        lo[ax], hi[ax], first[ax], last[ax] = 0, lat[k] - 1, 1, lat[k] - 2
        mm[tuple(lo)] = mm[tuple(last)]
        mm[tuple(hi)] = mm[tuple(first)]
    tmask = (1 << geo.NT_BITS[0]) - 1
    for z, y, x in zip(*np.nonzero((m & tmask) == geo.T_HALFBB)):
        m[z, y, x] = geo.encode(geo.T_HALFBB, orientation=geo.link_tags(grid, mm, z, y, x))


def inlet_params(frame):
    """The parameter table of open_channel: the inlet velocity (s U on the flow axis), then the outlet density."""
    a, s, b, c = axes(frame)
    vel = [0.0] * (2 if c is None else 3)
    vel[a] = s * U
    return vel + [1.0]


def force_of(frame):
    a, s, b, c = axes(frame)
    f = [0.0] * (2 if c is None else 3)
    f[a] = s * FORCE
    if c is not None:
        f[c] = FORCE_C
    return f


def initial_fields(frame, size):
    """rho = 1, u = s U along the flow axis on every node: every boundary works from the first step."""
    a, s, b, c = axes(frame)
    shape = tuple(reversed(size))
    v = [np.zeros(shape) for _ in size]
    v[a][...] = s * U
    return np.ones(shape), v


# ---- the cases -------------------------------------------------------------------------------------------------------
# name -> (kind, what, [(pattern, model, precision), ...]); what = (t_in, t_out, type table) of an open channel with
# full-way walls, or the walls of a forced duct
OPEN = {
    'zh': ('T_ZHVEL', 'T_ZHDENS', 'TYPE_KIND'),
    'reg': ('T_REGVEL', 'T_REGDENS', 'TYPE_KIND'),
    'eq': ('T_EQVEL', 'T_EQDENS', 'TYPE_KIND'),
    'copy': ('T_ZHVEL', 'T_COPY', 'TYPE_KIND_OUTFLOW'),
    'yu': ('T_ZHVEL', 'T_YU', 'TYPE_KIND_OUTFLOW'),
    'dn': ('T_ZHVEL', 'T_DONOTHING', 'TYPE_KIND_INPLACE'),
    # the same two with slip walls: every row of an x-flow frame then holds boundary-condition nodes
    'zh_slipwalls': ('T_ZHVEL', 'T_ZHDENS', 'TYPE_KIND_INPLACE'),
    'dn_slipwalls': ('T_ZHVEL', 'T_DONOTHING', 'TYPE_KIND_INPLACE'),
}
DUCT = {'slip': ('slip', 'TYPE_KIND_INPLACE'), 'hbb_tags': ('halfbb-tags', 'TYPE_KIND'),
        'hbb_orient': ('halfbb-orientation', 'TYPE_KIND')}

CASES_3D = [
    ('zh', 'AB', 'bgk', 'single'), ('reg', 'AA', 'mrt', 'single'), ('eq', 'AA', 'bgk', 'double'),
    ('copy', 'AB', 'bgk', 'single'), ('yu', 'AB', 'mrt', 'single'), ('yu', 'AB', 'bgk', 'double'),
    ('dn', 'AA', 'bgk', 'single'), ('dn', 'AA', 'mrt', 'single'),
    ('slip', 'AB', 'bgk', 'single'), ('slip', 'AA', 'bgk', 'single'), ('slip', 'AB', 'mrt', 'single'),
    ('slip', 'AA', 'mrt', 'single'),
    ('hbb_tags', 'AB', 'bgk', 'single'), ('hbb_tags', 'AA', 'bgk', 'single'),
    ('hbb_orient', 'AB', 'bgk', 'single'), ('hbb_orient', 'AA', 'bgk', 'single')]
# (not in the table of cases every frame test runs: for the row classes, tests/test_gpu_faces.py)
EXTRA_3D = [('zh_slipwalls', 'AB', 'bgk', 'single'), ('dn_slipwalls', 'AA', 'bgk', 'single')]
CASES_2D = [
    ('zh', 'AB', 'bgk', 'single'), ('reg', 'AA', 'mrt', 'single'), ('copy', 'AB', 'bgk', 'single'),
    ('yu', 'AB', 'mrt', 'single'), ('dn', 'AA', 'bgk', 'single'), ('dn', 'AA', 'mrt', 'single'),
    ('slip', 'AB', 'bgk', 'single'), ('slip', 'AA', 'bgk', 'single'), ('slip', 'AB', 'mrt', 'single'),
    ('slip', 'AA', 'mrt', 'single'), ('hbb_tags', 'AB', 'bgk', 'single'), ('hbb_tags', 'AA', 'bgk', 'single')]


def case_id(case):
    return '-'.join((case[0], case[1], case[2], 'f64' if case[3] == 'double' else 'f32'))


def setup(grid, frame, case, size, precision=None, out_normal=(-1, 0, 0)):
    """Everything tests/_pair.run_pair (or an OracleBox alone) needs for `case` in `frame`: (periodic, node_map_fn, init,
    desc keywords)."""
    name, pattern, model, prec = case
    a, s, b, c = axes(frame)
    dim = grid.dim
    kw = dict(model=model, precision=precision or prec, access_pattern=pattern, visc=VISC, fluid_only=False,
              nt_bits=geo.NT_BITS)
    periodic = [False] * 3
    if c is not None:
        periodic[c] = True
    if name in OPEN:
        t_in, t_out, table = OPEN[name]
        walls = 'slip' if name.endswith('slipwalls') else 'fullbb'
        kw.update(type_kind=getattr(geo, table), node_params=inlet_params(frame))

        def node_map_fn(desc):
            return open_channel(desc, frame, getattr(geo, t_in), getattr(geo, t_out), walls, grid, out_normal)
    else:
        walls, table = DUCT[name]
        periodic[a] = True
        kw.update(type_kind=getattr(geo, table), accel=force_of(frame), use_link_tags=walls != 'halfbb-orientation')

        def node_map_fn(desc):
            return forced_duct(desc, frame, walls, grid)
    kw['periodic_fused'] = [int(p) for p in periodic]
    return tuple(periodic), node_map_fn, initial_fields(frame, size), kw


def outlet_layer(field, frame, name):
    """The layer where the case's boundary of interest acts, of a real-node field in the x frame: the outlet layer of
    an open channel, the fluid layer next to the low wall of a duct."""
    return field[..., 1:-1, -1] if name in OPEN else field[..., 1, :]
