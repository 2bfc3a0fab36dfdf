"""numpy twin of the N-component Shan-Chen mixture, N = 2 (binary: csrc/slf_sc.hip, reference binary_shan_chen.mako) or
N = 3 (ternary: csrc/slf_sc3.hip, reference ternary_shan_chen.mako): the same operations in the same order, in float32 or
float64 (or longdouble, the wider format bounds are sized with).  tests/test_sc3_twin.py holds its pieces against the
reference's sympy objects (tests/golden/arith_sc3_*.npz) and, with N = 2, the whole of it against the CPU oracle bit for bit.

Dense arrays [Q] + shape with shape in numpy axis order ((z,) y, x), two-copy (AB) semantics, periodic along every axis;
`wall` marks full-way bounce-back nodes.  Operation order per step:

  pass in front, wet nodes:  rho_k = ((f_k,0 + f_k,1) + ...);  v = (1/tau_0) j_0, v = v + (1/tau_k) j_k for k = 1 ..;
                             total = ((1/tau_0) rho_0 + (1/tau_1) rho_1) [+ (1/tau_2) rho_2];  v = v / total
  sweep of lattice k:        S_j = sum_i psi(rho_j(x + e_i)) (+-w_i), i = 1 .. Q - 1, per component
                             a = 0;  for j with G_kj != 0:  a = a + S_j ((0 - psi(rho_k)) G_kj);  a = a / rho_k [+ body accel_k]
                             walls: f_i <-> f_opp(i);  wet: BGK with Guo forcing or the exact difference method;  stream
"""
import math

import numpy as np


def basis(grid):
    return [tuple(int(c) for c in e) for e in grid.basis]


def opposite(grid):
    b = basis(grid)
    return [b.index(tuple(-c for c in e)) for e in b]


def weights(grid, R):
    return [R(float(w)) for w in grid.weights]


_libm_exp = np.frompyfunc(math.exp, 1, 1)


def psi(rho, potential, R, exp='libm'):
    """sym.py:896-908: linear psi = rho, classic psi = 1 - exp(-rho).  exp: 'libm' -- the C library's double-precision exp
    on the argument widened to double, the result rounded to R (what the CPU oracle computes); 'numpy' -- numpy's exp in R."""
    rho = np.asarray(rho, dtype=R)
    if potential in (0, 'linear'):
        return rho
    arg = R(0) - rho
    if exp == 'libm' and R in (np.float32, np.float64):
        e = np.asarray(_libm_exp(arg.astype(np.float64)), dtype=np.float64).astype(R)
    else:
        e = np.exp(arg)
    return R(1) - e


def density(f):
    rho = f[0]
    for i in range(1, len(f)):
        rho = rho + f[i]
    return rho


def momentum(grid, f, d, R):
    acc = np.zeros_like(f[0])
    for i, e in enumerate(basis(grid)):
        if i == 0:
            continue
        if e[d] > 0:
            acc = acc + f[i]
        elif e[d] < 0:
            acc = acc - f[i]
    return acc


def edotv(e, v):
    acc = np.zeros_like(v[0])
    for c, vc in zip(e, v):
        if c > 0:
            acc = acc + vc
        elif c < 0:
            acc = acc - vc
    return acc


def usq15(v, R):
    s = v[0] * v[0] + v[1] * v[1]
    if len(v) == 3:
        s = s + v[2] * v[2]
    return R(1.5) * s


def feq(grid, rho, v, R, rho0=None):
    """bgk_equilibrium: w_i (rho + rho0 (eu (3 + 4.5 eu) - 1.5 u^2)), [Q, ...]."""
    rho = np.asarray(rho, dtype=R)
    rho0 = rho if rho0 is None else np.asarray(rho0, dtype=R)
    v = [np.asarray(c, dtype=R) for c in v]
    u15 = usq15(v, R)
    w = weights(grid, R)
    out = []
    for i, e in enumerate(basis(grid)):
        if i == 0:
            out.append(w[i] * (rho + rho0 * (R(0) - u15)))
        else:
            eu = edotv(e, v)
            out.append(w[i] * (rho + rho0 * (eu * (R(3) + R(4.5) * eu) - u15)))
    return np.array(out, dtype=R)


def guo_term(grid, rho, v, a, tau, R):
    """What Guo forcing adds to f_i: (rho pref) w_i ((e_i.a - v.a) + 3 (e_i.v) (e_i.a)) at the velocity v (= u + a / 2)."""
    pref = rho * R(3.0 * (1.0 - 0.5 / tau))
    va = v[0] * a[0] + v[1] * a[1]
    if len(v) == 3:
        va = va + v[2] * a[2]
    w = weights(grid, R)
    out = []
    for i, e in enumerate(basis(grid)):
        eu, ea = edotv(e, v), edotv(e, a)
        out.append(pref * w[i] * ((ea - va) + R(3) * eu * ea))
    return np.array(out, dtype=R)


def relax(grid, f, rho, v, a, tau, R, edm=False):
    """bgk_relax_accel (csrc/slf_node.h) with a force: returns the post-collision populations."""
    omega = R(1.0 / tau)
    if edm:
        vs = [vc + ac for vc, ac in zip(v, a)]
        fe, fs = feq(grid, rho, v, R), feq(grid, rho, vs, R)
        out = f + omega * (fe - f)
        return out + (fs - fe)
    v = [vc + R(0.5) * ac for vc, ac in zip(v, a)]
    fe = feq(grid, rho, v, R)
    out = f + omega * (fe - f)
    return out + guo_term(grid, rho, v, a, tau, R)


def stencil_sum(grid, psi_field, R):
    """S[d] = sum_i psi(x + e_i) (+-w_i) over the directions with e_i,d != 0, in index order; periodic."""
    b, w = basis(grid), weights(grid, R)
    dim = grid.dim
    axes = tuple(range(psi_field.ndim))
    S = [np.zeros_like(psi_field) for _ in range(dim)]
    for i in range(1, grid.Q):
        nb = np.roll(psi_field, tuple(-c for c in reversed(b[i])), axis=axes)      # value at x + e_i
        for d in range(dim):
            if b[i][d] > 0:
                S[d] = S[d] + nb * w[i]
            elif b[i][d] < 0:
                S[d] = S[d] + nb * (R(0) - w[i])
    return S


class ScTwin(object):
    def __init__(self, grid, shape, dtype, tau, G, potential='linear', accel=None, edm=False, wall=None, exp='libm'):
        """tau: N relaxation times; G: N x N couplings (G[k][j] couples lattice k to field j); accel: N body accelerations
        (dim components each) or None."""
        self.grid, self.shape, self.R = grid, tuple(shape), dtype
        self.n = len(tau)
        self.tau = [float(t) for t in tau]
        self.G = [[float(c) for c in row] for row in G]
        self.potential = potential
        self.accel = [[0.0] * grid.dim for _ in range(self.n)] if accel is None else [[float(c) for c in a] for a in accel]
        self.edm, self.exp = edm, exp
        self.wall = np.zeros(self.shape, dtype=bool) if wall is None else np.asarray(wall, dtype=bool)
        self.wet = ~self.wall
        self.f = [None] * self.n
        self.field = [None] * self.n
        self.v = None
        self.post = [None] * self.n      # populations of the last step after the collision, before streaming

    def astype(self, dtype):
        t = ScTwin(self.grid, self.shape, dtype, self.tau, self.G, self.potential, self.accel, self.edm, self.wall, self.exp)
        t.f = [f.astype(dtype) for f in self.f]
        t.field = [a.astype(dtype) for a in self.field]
        t.v = [a.astype(dtype) for a in self.v]
        return t

    def set_fields(self, fields, v):
        """SetInitialConditions: f_k = feq(field_k, v) on every node."""
        R = self.R
        self.field = [np.array(a, dtype=R) for a in fields]
        self.v = [np.array(a, dtype=R) for a in v]
        self.f = [feq(self.grid, a, self.v, R) for a in self.field]

    def macro(self):
        """The pass in front: densities and the common velocity of the wet nodes."""
        R, grid, wet = self.R, self.grid, self.wet
        rho, v, total = [], None, None
        with np.errstate(all='ignore'):
            for k in range(self.n):
                om = R(1.0 / self.tau[k])
                rho.append(density(self.f[k]))
                j = [om * momentum(grid, self.f[k], d, R) for d in range(grid.dim)]
                v = j if k == 0 else [a + b for a, b in zip(v, j)]
                total = om * rho[k] if k == 0 else total + om * rho[k]
            v = [a / total for a in v]
        self.field = [np.where(wet, a, b) for a, b in zip(rho, self.field)]
        self.v = [np.where(wet, a, b) for a, b in zip(v, self.v)]

    def accelerations(self):
        """a_k of every node (meaningful on wet nodes) from the fields as they are."""
        R, grid = self.R, self.grid
        p = [psi(a, self.potential, R, self.exp) for a in self.field]
        S = [stencil_sum(grid, a, R) for a in p]
        out = []
        with np.errstate(all='ignore'):
            for k in range(self.n):
                a = [np.zeros(self.shape, dtype=R) for _ in range(grid.dim)]
                for j in range(self.n):
                    cc = R(self.G[k][j])
                    if cc != 0:
                        a = [ad + S[j][d] * ((R(0) - p[k]) * cc) for d, ad in enumerate(a)]
                a = [ad / self.field[k] for ad in a]
                if any(c != 0.0 for c in self.accel[k]):
                    a = [ad + R(self.accel[k][d]) for d, ad in enumerate(a)]
                out.append(a)
        return out

    def step(self):
        R, grid = self.R, self.grid
        b, opp = basis(grid), opposite(grid)
        axes = tuple(range(len(self.shape)))
        self.macro()
        acc = self.accelerations()
        with np.errstate(all='ignore'):
            for k in range(self.n):
                f = self.f[k]
                bounced = f[opp]
                collided = relax(grid, f, self.field[k], self.v, acc[k], self.tau[k], R, self.edm)
                post = np.where(self.wall, bounced, np.where(self.wet, collided, f))
                self.post[k] = post
                self.f[k] = np.array([np.roll(post[i], tuple(reversed(b[i])), axis=axes) for i in range(grid.Q)], dtype=R)
