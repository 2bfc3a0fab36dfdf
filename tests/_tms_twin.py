"""numpy twin of the Tamm-Mott-Smith wall (NTWallTMS), test code only.

A restatement of what the reference's templates do at a TMS node (boundary.mako:631-648 fixMissingDistributions,
696-723 postcollisionBoundaryConditions, in the order of lb_single_fluid.mako:185-228) over a whole box of fluid nodes
and TMS walls, in the precision it is asked for and with the operation order of sailfish_amd/csrc/slf_node.h /
slf_sweep.h (macro_standard, macro_roundoff, feq, bgk_relax_accel, bgk_relax_roundoff, tms_fix_missing,
tms_add_equilibrium_difference):

    1. load the populations (two-copy: own slots; in place: own slots in even steps, pulled from the neighbours' opposite
       slots in odd ones);
    2. target state (tg_rho, tg_v) = the standard moments of what was loaded; every unknown population becomes
       feq_i(tg_rho, tg_v);
    3. instantaneous rho, v from the repaired populations;
    4. the collision of a wet node (BGK with optional Guo force here; `collide`: any other, one node at a time);
    5. f_i += feq_i(tg_rho, tg_v) for all i, then f_i -= feq_i(rho, v) for all i, v as the relaxation left it; then the
       half-way bounce-back store: for every direction i that points to a non-fluid node the reflected f_i goes where the
       node's next step reads its unknown population opp(i);
    6. propagate.

The arrays carry the layer of ghost nodes the kernels' arrays have ([Q, (lat_nz,) lat_ny, lat_nx], no x padding), so that
the in-place pattern can be restated slot for slot: its even step stores the reflected populations into the ghost (or
wall-side) nodes.  Periodic axes wrap between the first and the last real node.  The three density forms: 'compressible',
'incompressible', 'roundoff' (the arrays then hold f_i - w_i and the density variable is rho - 1)."""
from fractions import Fraction

import numpy as np

from tests._elbm_twin import _edotv, macros


def _wide(R):
    return np.finfo(R).eps < np.finfo(np.float64).eps


def _grid_tables(grid, R):
    """Direction vectors and weights.  float32 / float64: the weights as the kernels form them, (R)((double)num / den)
    (slf_node.h Weights); a wider format (the yardstick of the twin's own rounding error): num / den in that format."""
    e = np.array([list(v) + [0] * (3 - grid.dim) for v in grid.basis], dtype=np.int64)
    fr = [Fraction(x) for x in grid.weights]
    w = [R(x.numerator) / R(x.denominator) for x in fr] if _wide(R) else [R(float(x)) for x in fr]
    return e, w, None


def _rates(tau, R):
    """omega = 1 / tau and the Guo prefactor 3 (1 - 1 / (2 tau)): rounded from double like slf_sweep.h make_params, or formed
    in the wider format."""
    if _wide(R):
        return R(1) / R(tau), R(3) * (R(1) - R(0.5) / R(tau))
    return R(1.0 / tau), R(3.0 * (1.0 - 0.5 / tau))


def feq(grid, rho, rho0, v):
    """w_i (rho + rho0 (eu (3 + 4.5 eu) - 1.5 u^2)) with the second density given: slf_node.h feq."""
    R = rho.dtype.type
    e, w, _ = _grid_tables(grid, R)
    s = v[0] * v[0] + v[1] * v[1]
    if grid.dim == 3:
        s = s + v[2] * v[2]
    u15 = R(1.5) * s
    out = []
    for i in range(grid.Q):
        if not e[i].any():
            out.append(w[i] * (rho + rho0 * (R(0) - u15)))
        else:
            eu = _edotv(e, i, v, grid.dim)
            out.append(w[i] * (rho + rho0 * (eu * (R(3) + R(4.5) * eu) - u15)))
    return np.array(out)


def moments(grid, f, density):
    """The density variable and the velocity of the columns of f in the module's density form (macro_standard,
    macro_roundoff) and the equilibrium's second density."""
    R = f.dtype.type
    if density == 'roundoff':
        rho, j = macros(grid, f, incompressible=True)
        rho0 = rho + R(1)
        v = [c / rho0 for c in j[:grid.dim]] + j[grid.dim:]
        return rho, v, rho0
    inc = density == 'incompressible'
    rho, v = macros(grid, f, incompressible=inc)
    return rho, v, (np.ones_like(rho) if inc else rho)


def bgk_collide(grid, f, rho, v, rho0, tau, accel=None, density='compressible'):
    """bgk_relax_accel / bgk_relax_roundoff with Guo forcing or none.  Returns (post-collision f, output velocity).
    (The Guo term carries the density: rho, under 'roundoff' rho + 1.)"""
    R = f.dtype.type
    e, w, _ = _grid_tables(grid, R)
    omega, guo_pref = _rates(tau, R)
    v = list(v)
    a = None
    if accel is not None:
        a = [R(x) for x in accel] + [R(0)] * (3 - len(accel))
        for d in range(grid.dim):
            v[d] = v[d] + R(0.5) * a[d]
    fe = feq(grid, rho, rho0, v)
    out = f + omega * (fe - f)
    if a is not None:
        pref = (rho0 if density == 'roundoff' else rho) * guo_pref
        va = v[0] * a[0] + v[1] * a[1]
        if grid.dim == 3:
            va = va + v[2] * a[2]
        rows = []
        for i in range(grid.Q):
            eu = _edotv(e, i, v, grid.dim)
            ea = _edotv(e, i, a, grid.dim)
            if eu is None:
                eu, ea = np.zeros_like(rho), R(0)
            t = (ea - va) + R(3) * eu * ea
            rows.append(out[i] + pref * w[i] * t)
        out = np.array(rows)
    return out, v


def tms_node(grid, f, missing, density, collide):
    """Steps 2-5 (without the store) on the columns of f [Q, n]; missing [Q, n]: direction i of the node points to a
    non-fluid node, so population opp(i) is unknown.  collide(f, rho, v, rho0) -> (f, v_out).
    Returns dict(tg_rho, tg_v, repaired, rho, v, v_out, collided, post)."""
    opp = grid.idx_opposite
    tg_rho, tg_v, tg_rho0 = moments(grid, f, density)
    fe_tg = feq(grid, tg_rho, tg_rho0, tg_v)
    rep = f.copy()
    for i in range(1, grid.Q):
        rep[opp[i]] = np.where(missing[i], fe_tg[opp[i]], rep[opp[i]])
    rho, v, rho0 = moments(grid, rep, density)
    col, v_out = collide(rep, rho, v, rho0)
    post = col + fe_tg
    post = post - feq(grid, rho, rho0, v_out)
    return dict(tg_rho=tg_rho, tg_v=tg_v, repaired=rep, rho=rho, v=v, v_out=v_out, collided=col, post=post)


def missing_from_orientation(grid, orientation):
    """[Q, n] from orientation codes (1 .. 2 dim: the direction of the inward normal): direction i is missing iff
    e_i . n < 0 (sym.get_missing_dists for opp(i))."""
    e = np.array(grid.basis, dtype=np.int64)
    orientation = np.asarray(orientation)
    out = np.zeros((grid.Q,) + orientation.shape, dtype=bool)
    for o in range(1, 2 * grid.dim + 1):
        n = np.array(grid.dir_to_vec(o), dtype=np.int64)
        for i in range(1, grid.Q):
            if int(e[i].dot(n)) < 0:
                out[i] |= orientation == o
    return out


def missing_from_tags(grid, tags):
    """[Q, n] from link-tag words: bit i - 1 clear = direction i points to a non-fluid node."""
    tags = np.asarray(tags, dtype=np.int64)
    out = np.zeros((grid.Q,) + tags.shape, dtype=bool)
    for i in range(1, grid.Q):
        out[i] = ((tags >> (i - 1)) & 1) == 0
    return out


class TmsTwin(object):
    """A box of wet nodes.  f: [Q, (lat_nz,) lat_ny, lat_nx] with the ghost layer; tms: bool over the lattice, True on the
    TMS nodes (real nodes only; every other real node is fluid unless `dry` says it takes no part); missing: [Q, lattice]
    (missing_from_tags / missing_from_orientation; read on TMS nodes only); periodic: per axis (x, y[, z])."""

    def __init__(self, grid, f, tms, missing, visc, periodic, pattern='AB', density='compressible', accel=None,
                 collide=None, dry=None):
        self.grid, self.pattern, self.density = grid, pattern, density
        self.dtype = np.asarray(f).dtype
        self.lat = np.asarray(f).shape[1:]
        self.tau = (6.0 * visc + 1.0) / 2.0
        self.accel = accel
        self._collide = collide
        nd = len(self.lat)
        self.dist = [np.array(f).reshape(grid.Q, -1)]
        if pattern == 'AB':
            self.dist.append(self.dist[0].copy())
        self.iteration = 0
        real = np.zeros(self.lat, dtype=bool)
        real[tuple(slice(1, n - 1) for n in self.lat)] = True
        if dry is not None:
            real &= ~np.asarray(dry, dtype=bool)
        coords = np.argwhere(real)                                   # array axes are (z,) y, x
        self.own = np.ravel_multi_index(tuple(coords.T), self.lat)
        self.is_tms = np.asarray(tms, dtype=bool).reshape(-1)[self.own]
        self.missing = np.asarray(missing, dtype=bool).reshape(grid.Q, -1)[:, self.own] & self.is_tms[None, :]
        self.nbr_p, self.nbr_m = [], []
        for i in range(grid.Q):
            e = grid.basis[i]
            for sign, store in ((1, self.nbr_p), (-1, self.nbr_m)):
                c = coords.copy()
                for ax in range(nd):                                 # lattice axis ax = array axis nd - 1 - ax
                    k, n = nd - 1 - ax, self.lat[nd - 1 - ax]
                    c[:, k] += sign * e[ax]
                    if periodic[ax]:
                        c[:, k] = np.where(c[:, k] > n - 2, 1, np.where(c[:, k] < 1, n - 2, c[:, k]))
                store.append(np.ravel_multi_index(tuple(c.T), self.lat))
        self.rho = np.zeros(self.lat, dtype=self.dtype)
        self.v = [np.zeros(self.lat, dtype=self.dtype) for _ in range(grid.dim)]
        self.loaded = self.post = None

    def collide(self, f, rho, v, rho0):
        if self._collide is not None:
            return self._collide(f, rho, v, rho0)
        return bgk_collide(self.grid, f, rho, v, rho0, self.tau, self.accel, self.density)

    def current(self):
        """The populations as the arrays hold them now, [Q, lattice]."""
        idx = 0 if self.pattern == 'AA' else (self.iteration & 1)
        return self.dist[idx].reshape((self.grid.Q,) + self.lat)

    def step(self):
        g, Q, opp = self.grid, self.grid.Q, self.grid.idx_opposite
        odd = self.pattern == 'AA' and (self.iteration & 1) == 1
        even = self.pattern == 'AA' and not odd
        src = self.dist[0] if self.pattern == 'AA' else self.dist[self.iteration & 1]
        dst = self.dist[0] if self.pattern == 'AA' else self.dist[1 - (self.iteration & 1)]
        if odd:
            f = np.array([src[opp[i]][self.nbr_m[i]] for i in range(Q)])
        else:
            f = np.array([src[i][self.own] for i in range(Q)])
        self.loaded = f.copy()
        t = self.is_tms
        post = np.empty_like(f)
        rho = np.empty(f.shape[1], dtype=f.dtype)
        v_out = [np.empty(f.shape[1], dtype=f.dtype) for _ in range(3)]
        v_in = [np.empty(f.shape[1], dtype=f.dtype) for _ in range(3)]
        if (~t).any():
            r, v, r0 = moments(g, f[:, ~t], self.density)
            post[:, ~t], vo = self.collide(f[:, ~t], r, v, r0)
            rho[~t] = r
            for d in range(3):
                v_out[d][~t] = vo[d]
                v_in[d][~t] = v[d]
        if t.any():
            n = tms_node(g, f[:, t], self.missing[:, t], self.density, self.collide)
            post[:, t] = n['post']
            rho[t] = n['rho']
            for d in range(3):
                v_out[d][t] = n['v_out'][d]
                v_in[d][t] = n['v'][d]
        self.post = post
        self.rho.reshape(-1)[self.own] = rho
        for d in range(g.dim):
            self.v[d].reshape(-1)[self.own] = v_out[d]
        for i in range(Q):
            if even:
                dst[opp[i]][self.own] = post[i]
            else:
                dst[i][self.nbr_p[i]] = post[i]
        for i in range(1, Q):
            m = self.missing[i]
            if even:
                dst[i][self.nbr_p[i][m]] = post[i][m]
            else:
                dst[opp[i]][self.own[m]] = post[i][m]
        self.iteration += 1

    def run(self, n):
        for _ in range(n):
            self.step()
        return self
