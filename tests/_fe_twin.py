"""numpy twin of the free-energy binary fluid (sailfish_amd/csrc/slf_fe.hip; reference lb_binary.py:139-372,
templates/models/lb_binary_fluid.mako, sym_equilibrium.py:15-71, finite_difference_optimized.mako): the same operations
in the same order, in any numpy floating-point format -- float32 / float64 as the kernels, longdouble as the wider
format the GPU tests size their bounds with.  tests/test_fe_twin.py holds it against the reference's sympy objects
(tests/golden/arith_fe_*.npz).

Arrays are [Q] + shape with shape in numpy axis order ((z,) y, x); a box is periodic along every axis unless both rim
layers of the axis are dry (walls), in which case nothing a wet node reads ever crosses the rim.
"""
import numpy as np


def basis(grid):
    """e_i as integer tuples (x, y[, z]) in the kernels' direction order."""
    return [tuple(int(c) for c in e) for e in grid.basis]


def opposite(grid):
    b = basis(grid)
    return [b.index(tuple(-c for c in e)) for e in b]


def weight_tables(grid):
    """wi, wxx, wyy, wzz, wxy, wyz, wxz of reference lb_binary.py:198-268 for directions 1 .. Q - 1 (floats)."""
    out = dict((k, []) for k in ('wi', 'wxx', 'wyy', 'wzz', 'wxy', 'wyz', 'wxz'))
    for e in basis(grid)[1:]:
        e3 = tuple(e) + (0,) * (3 - len(e))
        axis = sum(c * c for c in e3) == 1
        if grid.dim == 3:
            out['wi'].append(1.0 / 6.0 if axis else 1.0 / 12.0)
            waa = [(5.0 / 12.0 if c else -1.0 / 3.0) if axis else (-1.0 / 24.0 if c else 1.0 / 12.0) for c in e3]
        else:
            out['wi'].append(1.0 / 3.0 if axis else 1.0 / 12.0)
            waa = [(1.0 / 3.0 if c else -1.0 / 6.0) if axis else -1.0 / 24.0 for c in e3[:2]] + [0.0]
        out['wxx'].append(waa[0]); out['wyy'].append(waa[1]); out['wzz'].append(waa[2])
        out['wxy'].append(0.25 * e3[0] * e3[1]); out['wyz'].append(0.25 * e3[1] * e3[2]); out['wxz'].append(0.25 * e3[0] * e3[2])
    return out


def _edotv(e, v):
    acc = None
    for c, vc in zip(e, v):
        if c > 0:
            acc = vc if acc is None else acc + vc
        elif c < 0:
            acc = -vc if acc is None else acc - vc
    return acc


def _h(eu, husq, R):
    return (eu + R(1.5) * (eu * eu)) - husq


def _half_usq(v, R):
    s = v[0] * v[0] + v[1] * v[1]
    if len(v) == 3:
        s = s + v[2] * v[2]
    return R(0.5) * s


def feq_fluid(grid, rho, phi, lap, v, grad, A, kappa, dtype):
    """free_energy_equilibrium_fluid: [Q, ...]."""
    R = dtype
    rho, phi, lap = (np.asarray(a, dtype=R) for a in (rho, phi, lap))
    v = [np.asarray(c, dtype=R) for c in v]
    grad = [np.asarray(c, dtype=R) for c in grad]
    A, kappa = R(A), R(kappa)
    w = weight_tables(grid)
    phi2 = phi * phi
    pb = rho / R(3) + A * (phi2 * (R(0.75) * phi2 - R(0.5)))
    bulk = pb - (kappa * phi) * lap
    husq = _half_usq(v, R)
    gg = [g * g for g in grad]
    out = [None]
    total = None
    for k, e in enumerate(basis(grid)[1:]):
        eu = _edotv(e, v)
        q = R(w['wxx'][k]) * gg[0] + R(w['wyy'][k]) * gg[1]
        if grid.dim == 3:
            q = q + R(w['wzz'][k]) * gg[2]
        e3 = tuple(e) + (0,) * (3 - len(e))
        if e3[0] * e3[1]:
            q = q + R(w['wxy'][k]) * (grad[0] * grad[1])
        if e3[1] * e3[2]:
            q = q + R(w['wyz'][k]) * (grad[1] * grad[2])
        if e3[0] * e3[2]:
            q = q + R(w['wxz'][k]) * (grad[0] * grad[2])
        t = R(w['wi'][k]) * (bulk + rho * _h(eu, husq, R)) + kappa * q
        out.append(t)
        total = t if total is None else total + t
    out[0] = rho - total
    return np.array(out, dtype=R)


def feq_order(grid, phi, lap, v, A, kappa, Gamma, dtype):
    """free_energy_equilibrium_order_param: [Q, ...]."""
    R = dtype
    phi, lap = np.asarray(phi, dtype=R), np.asarray(lap, dtype=R)
    v = [np.asarray(c, dtype=R) for c in v]
    A, kappa, Gamma = R(A), R(kappa), R(Gamma)
    w = weight_tables(grid)
    phi2 = phi * phi
    gmu = Gamma * (A * (phi * phi2 - phi) - kappa * lap)
    husq = _half_usq(v, R)
    out = [None]
    total = None
    for k, e in enumerate(basis(grid)[1:]):
        t = R(w['wi'][k]) * (gmu + phi * _h(_edotv(e, v), husq, R))
        out.append(t)
        total = t if total is None else total + t
    out[0] = phi - total
    return np.array(out, dtype=R)


def tau0(phi, tau_a, tau_b, dtype):
    """relaxation_common.mako:156-163."""
    R = dtype
    phi = np.asarray(phi, dtype=R)
    t = R(tau_b) + ((phi + R(1)) * (R(tau_a) - R(tau_b))) * R(0.5)
    return np.where(phi < R(-1), R(tau_b), np.where(phi > R(1), R(tau_a), t)).astype(R)


def stencil(grid, at, c, dtype):
    """laplacian_and_grad (finite_difference_optimized.mako:20-48): at(i) = the field at x + e_i, c = at x.
    Returns lap, [grad]."""
    R = dtype
    if grid.dim == 3:
        fe, fw, fn, fs, ft, fb = (at(i) for i in range(1, 7))
        fne, fnw, fse, fsw = (at(i) for i in range(7, 11))
        ftn, fts, fbn, fbs = (at(i) for i in range(11, 15))
        fte, ftw, fbe, fbw = (at(i) for i in range(15, 19))
        gx = ((((((((-fnw) - fsw) - ftw) - fbw) + fse) + fne) + fte) + fbe) / R(12) + (fe - fw) / R(6)
        gy = ((((((((-fse) - fsw) - fts) - fbs) + fne) + fnw) + ftn) + fbn) / R(12) + (fn - fs) / R(6)
        gz = ((((((((-fbe) - fbw) - fbn) - fbs) + fte) + ftw) + ftn) + fts) / R(12) + (ft - fb) / R(6)
        lap = (((((((((((fnw + fne) + fse) + fsw) + fte) + ftw) + ftn) + fts) + fbe) + fbw) + fbn) + fbs) / R(6) + \
            (((((ft + fb) + fe) + fw) + fn) + fs) / R(3) - R(4) * c
        return lap, [gx, gy, gz]
    fe, fn, fw, fs, fne, fnw, fsw, fse = (at(i) for i in range(1, 9))
    gx = ((((-fnw) - fsw) + fse) + fne) / R(12) + (fe - fw) / R(3)
    gy = ((((-fse) - fsw) + fne) + fnw) / R(12) + (fn - fs) / R(3)
    lap = (((((fnw + fne) + fsw) + fse) + R(4) * (((fe + fw) + fn) + fs)) - R(20) * c) / R(6)
    return lap, [gx, gy]


def density(f):
    rho = f[0]
    for i in range(1, len(f)):
        rho = rho + f[i]
    return rho


def momentum(grid, f, d):
    acc = None
    for i, e in enumerate(basis(grid)):
        if e[d] > 0:
            acc = f[i] if acc is None else acc + f[i]
        elif e[d] < 0:
            acc = -f[i] if acc is None else acc - f[i]
    return acc


def collide(grid, f, g, phi, lap, grad, dtype, Gamma, kappa, A, tau_a, tau_b, tau_phi):
    """One collision of both lattices on states [Q, n] with the given phi, Laplacian and gradient: what the two sweeps do
    to a wet node.  Returns dict f, g, rho, v."""
    R = dtype
    f, g = np.asarray(f, dtype=R), np.asarray(g, dtype=R)
    rho = density(f)
    v = [momentum(grid, f, d) / rho for d in range(grid.dim)]
    fe = feq_fluid(grid, rho, phi, lap, v, grad, A, kappa, R)
    omega = R(1) / tau0(phi, tau_a, tau_b, R)
    f_new = f + omega * (fe - f)
    ge = feq_order(grid, phi, lap, v, A, kappa, Gamma, R)
    g_new = g + R(1.0 / tau_phi) * (ge - g)
    return {'f': f_new, 'g': g_new, 'rho': rho, 'v': v}


class FeTwin(object):
    """A box of the free-energy model, stepped as the three kernels step it.  wall: Boolean array (full-way bounce-back
    nodes), orientation: integer array (basis index of the wall's normal, 0 = none)."""

    def __init__(self, grid, shape, dtype=np.float64, Gamma=0.5, kappa=0.5, A=0.5, tau_a=1.0, tau_b=1.0, tau_phi=1.0,
                 wall=None, orientation=None, wall_order=2, wall_phase=0.0):
        self.grid, self.shape, self.R = grid, tuple(shape), dtype
        self.c = dict(Gamma=Gamma, kappa=kappa, A=A, tau_a=tau_a, tau_b=tau_b, tau_phi=tau_phi)
        self.wall = np.zeros(self.shape, dtype=bool) if wall is None else np.asarray(wall, dtype=bool)
        self.orientation = np.zeros(self.shape, dtype=int) if orientation is None else np.asarray(orientation)
        self.wall_order, self.wall_phase = int(wall_order), wall_phase
        self.wet = ~self.wall
        self.b, self.opp = basis(grid), opposite(grid)
        self.axes = tuple(range(len(self.shape)))
        self.iteration = 0

    def astype(self, dtype):
        """The same box and state in another floating-point format (values converted, not recomputed)."""
        t = FeTwin(self.grid, self.shape, dtype, wall=self.wall, orientation=self.orientation, wall_order=self.wall_order,
                   wall_phase=self.wall_phase, **self.c)
        t.f, t.g = self.f.astype(dtype), self.g.astype(dtype)
        t.rho, t.phi, t.lap = self.rho.astype(dtype), self.phi.astype(dtype), self.lap.astype(dtype)
        t.v = [c.astype(dtype) for c in self.v]
        t.iteration = self.iteration
        return t

    def _at(self, a, e, k=1):
        """a at x + k e."""
        return np.roll(a, tuple(-k * c for c in reversed(e)), axis=self.axes)

    def _stencil(self, phi):
        return stencil(self.grid, lambda i: self._at(phi, self.b[i]), phi, self.R)

    def set_fields(self, rho, phi, v):
        """SetInitialConditions: both lattices at their equilibria, Laplacian and gradient of the given phi."""
        R = self.R
        rho, phi = np.asarray(rho, dtype=R), np.asarray(phi, dtype=R)
        v = [np.asarray(c, dtype=R) for c in v]
        lap, grad = self._stencil(phi)
        # dry nodes start without gradient terms (their stencil may reach beyond the box)
        lap = np.where(self.wet, lap, R(0)).astype(R)
        grad = [np.where(self.wet, c, R(0)).astype(R) for c in grad]
        self.f = feq_fluid(self.grid, rho, phi, lap, v, grad, self.c['A'], self.c['kappa'], R)
        self.g = feq_order(self.grid, phi, lap, v, self.c['A'], self.c['kappa'], self.c['Gamma'], R)
        self.rho, self.phi, self.v, self.lap = rho.copy(), phi.copy(), [c.copy() for c in v], np.zeros(self.shape, dtype=R)

    def macro(self):
        """FreeEnergyPrepareMacroFields: phi of the wet nodes, then the wetting walls."""
        R = self.R
        formed = density(self.g)
        phi = np.where(self.wet, formed, self.phi).astype(R)
        shift = R(float(self.wall_order) * float(self.wall_phase))      # the product in double, then the kernel's format
        for o in np.unique(self.orientation[self.wall]):
            sel = self.wall & (self.orientation == o)
            src = self._at(formed, self.b[o], self.wall_order) if o else formed
            phi = np.where(sel, src - shift, phi).astype(R)
        self.phi = phi

    def step(self):
        R, grid, c = self.R, self.grid, self.c
        self.macro()
        lap, grad = self._stencil(self.phi)
        r = collide(grid, self.f, self.g, self.phi, lap, grad, R, **c)
        wet = self.wet
        self.rho = np.where(wet, r['rho'], self.rho).astype(R)
        self.v = [np.where(wet, a, b).astype(R) for a, b in zip(r['v'], self.v)]
        self.lap = np.where(wet, lap, self.lap).astype(R)
        for name in ('f', 'g'):
            old = getattr(self, name)
            post = np.where(wet, r[name], old[self.opp])            # walls: full-way bounce-back
            new = np.array([np.roll(post[i], tuple(reversed(e)), axis=self.axes) for i, e in enumerate(self.b)], dtype=R)
            setattr(self, name, new)
        self.iteration += 1

    def run(self, steps):
        for _ in range(steps):
            self.step()
