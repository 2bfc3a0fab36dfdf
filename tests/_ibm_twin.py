"""numpy twin of a time step with immersed boundary markers (device code: csrc/slf_ibm.hip behind the C ABI's
slf_ibm_* entry points): tests/_accf_twin.AccfTwinBox for the fluid step, composed with the marker arithmetic, which is
restated here independently of the kernel file -- arrays over the markers, one numpy operation per floating-point
operation, in the module's format R:

    i0[d] = (int)floor(x[d]);  the stencil is the 2^dim nodes i0[d] + {0, 1}, z outermost, x innermost
    w[d]  = 1 - |x[d] - (R)i[d]|;  w = wx * wy (2-D), (wx * wy) * wz (3-D)
    spread:  c = ((-k) * (x[d] - ref[d])) * w;  q = llrint((double)c * 2^48);  acc[d][node] += q   (int64: exact, any order)
    gather:  field[d][node] = (R)((double)acc[d][node] * 2^-48)                                    (stencil nodes only)
    the fluid step, storing rho and v
    clear:   acc[d][node] = 0, field[d][node] = 0                                                  (stencil nodes only)
    advect:  v_p[d] = 0, then in stencil order v_p[d] = v_p[d] + w * (v[d][node] if the node is wet else 0);  x[d] += v_p[d]

A stencil node that is not a real node of the subdomain is skipped everywhere; a marker that has one does not move and is
counted in `outside`.  Positions are global lattice coordinates; `origin` is the global coordinate of the first real node.
Test-only."""
import numpy as np

from sailfish_amd import hipabi
from tests import _lat_twin as lt
from tests._accf_twin import AccfTwinBox

SCALE = 2.0 ** 48


class IbmTwinBox(AccfTwinBox):
    def __init__(self, desc, periodic, node_map, position, ref_position, stiffness, origin=(0, 0, 0), fill=np.nan):
        """position, ref_position: [n, dim]; stiffness: [n].  The field starts as 0 at the real nodes and `fill` everywhere
        else (no launch may read or write those entries)."""
        shape = tuple(reversed([desc.lat_nx - 2, desc.lat_ny - 2] + ([desc.lat_nz - 2] if desc.lattice != hipabi.SLF_D2Q9 else [])))
        dim = len(shape)
        super(IbmTwinBox, self).__init__(desc, periodic, node_map, accel_field=np.zeros((dim,) + shape), fill=fill)
        R = self.dtype
        self.pos = np.ascontiguousarray(np.asarray(position, dtype=np.float64).reshape(-1, dim).T, dtype=R)       # [dim, n]
        self.ref = np.ascontiguousarray(np.asarray(ref_position, dtype=np.float64).reshape(-1, dim).T, dtype=R)
        self.k = np.asarray(stiffness, dtype=np.float64).astype(R)
        self.n = self.pos.shape[1]
        self.origin = [int(x) for x in origin] + [0] * (3 - len(origin))
        self.acc = np.zeros((dim,) + self.shape, dtype=np.int64)
        self.outside = 0
        self.quantised = []          # the q of the last spread(), one array per (stencil node, component), valid lanes only
        d = desc
        if d.fluid_only or self.node_map is None:
            self.wet = np.ones(self.shape, dtype=bool)
        else:
            kind = np.array(list(d.type_kind[:d.n_types]))[self.node_map & np.uint32(d.nt_type_mask)]
            self.wet = np.isin(kind, lt.WET)

    def stencil(self):
        """[(valid [n] bool, (z, y, x) index arrays [n] (clipped where not valid), weight [n] in R)] in stencil order, and
        inside [n]: every node of the marker's stencil is a real node."""
        R, dim, d = self.dtype, self.dim, self.desc
        lat = [d.lat_nx, d.lat_ny, d.lat_nz]
        arr = [d.arr_nx, d.arr_ny, d.arr_nz]
        ok, w, a0 = [], [], []
        inside = np.ones(self.n, dtype=bool)
        for k in range(dim):
            x = self.pos[k]
            finite = (x >= R(-2.0 ** 30)) & (x <= R(2.0 ** 30))
            i0 = np.floor(np.where(finite, x, R(0))).astype(np.int64)
            a = i0 - self.origin[k] + 1
            a0.append(a)
            ok.append([finite & (a + o >= 1) & (a + o <= lat[k] - 2) for o in (0, 1)])
            w.append([R(1) - np.abs(x - (i0 + o).astype(R)) for o in (0, 1)])
            inside &= ok[k][0] & ok[k][1]
        out = []
        for oz in ((0, 1) if dim == 3 else (0,)):
            for oy in (0, 1):
                for ox in (0, 1):
                    valid = ok[0][ox] & ok[1][oy]
                    wt = w[0][ox] * w[1][oy]
                    if dim == 3:
                        valid = valid & ok[2][oz]
                        wt = wt * w[2][oz]
                    idx = (np.clip(a0[2] + oz, 0, arr[2] - 1) if dim == 3 else np.zeros(self.n, dtype=np.int64),
                           np.clip(a0[1] + oy, 0, arr[1] - 1), np.clip(a0[0] + ox, 0, arr[0] - 1))
                    out.append((valid, idx, wt.astype(R)))
        return out, inside

    def spread(self):
        R = self.dtype
        nodes, _ = self.stencil()
        self.quantised = []
        nk = -self.k
        with np.errstate(all='ignore'):
            for valid, idx, wt in nodes:
                at = tuple(c[valid] for c in idx)
                for k in range(self.dim):
                    c = ((nk * (self.pos[k] - self.ref[k])) * wt).astype(R)
                    q = np.rint(c.astype(np.float64) * SCALE)[valid].astype(np.int64)
                    np.add.at(self.acc[k], at, q)
                    self.quantised.append((k, q))

    def gather(self):
        R = self.dtype
        nodes, _ = self.stencil()
        for valid, idx, _ in nodes:
            at = tuple(c[valid] for c in idx)
            for k in range(self.dim):
                self.accel_field[k][at] = (self.acc[k][at].astype(np.float64) * (1.0 / SCALE)).astype(R)

    def clear_and_advect(self):
        R = self.dtype
        nodes, inside = self.stencil()
        vp = np.zeros((self.dim, self.n), dtype=R)
        with np.errstate(all='ignore'):
            for valid, idx, wt in nodes:
                at = tuple(c[valid] for c in idx)
                wet = self.wet[at]
                for k in range(self.dim):
                    self.acc[k][at] = 0
                    self.accel_field[k][at] = R(0)
                    vn = np.where(wet, self.v[k][at], R(0)).astype(R)
                    vp[k, valid] = vp[k, valid] + wt[valid] * vn
            self.last_vp = vp
            self.pos[:, inside] = self.pos[:, inside] + vp[:, inside]
        self.outside = int((~inside).sum())

    def step(self, save_macro=True, region=None):
        assert save_macro and region is None         # the markers read v after every step
        self.spread()
        self.gather()
        super(IbmTwinBox, self).step(save_macro=True)
        self.clear_and_advect()

    def positions(self):
        return np.array(self.pos.T)
