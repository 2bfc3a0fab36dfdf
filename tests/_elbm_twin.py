"""numpy twin of the entropic collision (--model=elbm), test code only.

A restatement of the reference's algorithm (templates/entropic.mako, relaxation.mako:56-97 ELBM_relaxate,
sym_equilibrium.py:123-223, sym.alpha_series) vectorised over nodes, in the precision it is asked for and with the
operation order of sailfish_amd/csrc/slf_node.h (elbm_fneq, elbm_relax, elbm_newton), so that in the same precision it
takes the same branches as the kernels:

    fneq = feq - f                       feq: the BGK polynomial, or the product form (entropic_eq)
    dev  = max_i |fneq_i / f_i|
    dev < 1e-6: alpha = 2;  dev < 0.01: the series in a1..a4;  otherwise Newton on H(f + alpha fneq) = H(f),
    H(f) = sum_i f_i (ln f_i - ln w_i), started from the node's previous alpha
    f += alpha beta fneq,  beta = 1 / (2 tau0 + 1),  tau0 = visc / cs^2

`log2=True` computes ln x as log2(x) ln 2: an equally valid implementation, used to measure how far two of them may
drift apart.  ElbmTwin steps a whole box: collision on the fluid nodes, full-way bounce-back on the wall nodes, periodic
streaming."""
import math

import numpy as np

LN2 = 0.6931471805599453


def _grid_tables(grid, R):
    e = np.array([list(v) + [0] * (3 - grid.dim) for v in grid.basis], dtype=np.int64)
    w = [R(float(x)) for x in grid.weights]
    nlw = [R(-math.log(float(x))) for x in grid.entropic_weights]
    return e, w, nlw


def macros(grid, f, incompressible=False):
    """rho, v[3] in the kernels' summation order (slf_node.h: density, momentum, macro_standard)."""
    R = f.dtype.type
    e, _, _ = _grid_tables(grid, R)
    rho = f[0].copy()
    for i in range(1, grid.Q):
        rho = rho + f[i]
    v = []
    for d in range(3):
        acc = np.zeros_like(rho)
        for i in range(1, grid.Q):
            if e[i, d] > 0:
                acc = acc + f[i]
            elif e[i, d] < 0:
                acc = acc - f[i]
        v.append(acc)
    if not incompressible:
        v = [c / rho for c in v[:grid.dim]] + v[grid.dim:]
    return rho, v


def _edotv(e, i, v, dim):
    """e_i . v, components in x, y, z order (slf_node.h edotv: 0 + v and 0 - v are exact)."""
    acc = None
    for d in range(dim):
        if e[i, d] > 0:
            acc = v[d] if acc is None else acc + v[d]
        elif e[i, d] < 0:
            acc = -v[d] if acc is None else acc - v[d]
    return acc


def feq_bgk(grid, rho, v, incompressible=False):
    """w_i (rho + rho0 (eu (3 + 4.5 eu) - 1.5 u^2)): slf_node.h feq."""
    R = rho.dtype.type
    e, w, _ = _grid_tables(grid, R)
    rho0 = np.ones_like(rho) if incompressible else rho
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


def feq_entropic(grid, rho, v):
    """The product form: D2Q9 sym_equilibrium.elbm_equilibrium, D3Q19 elbm_d3q19_equilibrium at order 8
    (slf_node.h elbm_fneq<.., true>)."""
    R = rho.dtype.type
    e, w, _ = _grid_tables(grid, R)
    c, ic = [], []
    if grid.dim == 2:
        pref = rho
        for d in range(2):
            s = np.sqrt(R(1) + R(3) * (v[d] * v[d]))
            pref = pref * (R(2) - s)
            c.append((R(2) * v[d] + s) / (R(1) - v[d]))
            ic.append(R(1) / c[d])
    else:
        x2, y2, z2 = v[0] * v[0], v[1] * v[1], v[2] * v[2]
        q = [x2, y2, z2]
        x4, y4, z4 = x2 * x2, y2 * y2, z2 * z2
        vsq = (x2 + y2) + z2
        yz, y2z2, y4z4 = y2 + z2, y2 * z2, y4 + z4
        o6 = ((x4 * x2 + x4 * yz) + yz * y4z4) + x2 * ((y4 + R(12) * y2z2) + z4)
        o8 = (((((((R(5) * (x4 * x4) + R(5) * (y4 * y4)) + R(4) * (y4 * y2) * z2) + R(2) * y4 * z4) +
                 R(4) * y2 * (z4 * z2)) + R(5) * (z4 * z4)) + R(4) * (x4 * x2) * yz) +
              (R(4) * x2 * yz * ((y4 + R(17) * y2z2) + z4) + R(2) * x4 * ((y4 + R(36) * y2z2) + z4)))
        pref = rho * ((((R(1) - R(1.5) * vsq) + R(1.125) * (vsq * vsq)) - R(1.6875) * o6) + R(0.6328125) * o8)
        for d in range(3):
            a, a2 = v[d], q[d]
            b2c2, bpc = q[(d + 1) % 3] * q[(d + 2) % 3], q[(d + 1) % 3] + q[(d + 2) % 3]
            a3, a4 = a2 * a, a2 * a2
            a6 = a4 * a2
            t = (((R(1) + R(3) * a) + R(4.5) * a2) + R(4.5) * a3) + R(3.375) * a4
            t = t + R(3.375) * (a4 * a + R(2) * a * b2c2)
            t = t + R(5.0625) * (a6 + R(4) * a2 * b2c2)
            t = t + R(5.0625) * (a * ((a6 + R(4) * a2 * b2c2) - b2c2 * bpc))
            t = t + R(1.8984375) * (a2 * (a6 - R(8) * b2c2 * bpc))
            c.append(t)
            ic.append(R(1) / t)
    out = []
    for i in range(grid.Q):
        t = pref * w[i]
        for d in range(grid.dim):
            if e[i, d] > 0:
                t = t * c[d]
            elif e[i, d] < 0:
                t = t * ic[d]
        out.append(t)
    return np.array(out)


def a_coeffs(f, fneq):
    """dev and a1..a4 in one pass (ComputeACoeff / SmallEquilibriumDeviation; slf_node.h elbm_relax); a1..a4 WITHOUT the
    factors 1/2, -1/6, 1/12, -1/20."""
    R = f.dtype.type
    dev = np.zeros_like(f[0])
    a = [np.zeros_like(f[0]) for _ in range(4)]
    with np.errstate(all='ignore'):
        for i in range(f.shape[0]):
            inv = R(1) / f[i]
            t = fneq[i] * inv
            p = fneq[i] * fneq[i] * inv
            at = np.abs(t)
            dev = np.where(at > dev, at, dev)
            a[0] = a[0] + p
            for k in (1, 2, 3):
                p = p * t
                a[k] = a[k] + p
    return dev, a


def alpha_series(a1, a2, a3, a4):
    """sym.alpha_series() on the coefficients WITH their factors (the reference's a1..a4)."""
    R = np.asarray(a1).dtype.type
    i1 = R(1) / a1
    x2, x3, x4 = a2 * i1, a3 * i1, a4 * i1
    return ((((((R(2) - R(4) * x2) + R(16) * (x2 * x2)) - R(8) * x3) + R(80) * (x2 * x3)) - R(80) * (x2 * x2 * x2)) -
            R(16) * x4)


def _series_from_raw(a):
    R = a[0].dtype.type
    i1 = R(1) / (R(0.5) * a[0])
    x2, x3, x4 = (R(-1.0 / 6.0) * a[1]) * i1, (R(1.0 / 12.0) * a[2]) * i1, (R(-1.0 / 20.0) * a[3]) * i1
    return ((((((R(2) - R(4) * x2) + R(16) * (x2 * x2)) - R(8) * x3) + R(80) * (x2 * x3)) - R(80) * (x2 * x2 * x2)) -
            R(16) * x4)


def _ln(x, log2):
    R = x.dtype.type
    with np.errstate(all='ignore'):
        return np.log2(x) * R(LN2) if log2 else np.log(x)


def entropy(grid, f, log2=False):
    """H(f) = sum_i f_i (ln f_i - ln w_i) (CalculateEntropy)."""
    R = f.dtype.type
    _, _, nlw = _grid_tables(grid, R)
    ent = np.zeros_like(f[0])
    with np.errstate(all='ignore'):
        for i in range(grid.Q):
            ent = ent + f[i] * (_ln(f[i], log2) + nlw[i])
    return ent


def max_alpha(f, fneq):
    """FindMaxAlpha: the largest alpha that keeps every population of f + alpha fneq positive, at most 1000."""
    R = f.dtype.type
    m = np.full_like(f[0], R(1000))
    with np.errstate(all='ignore'):
        for i in range(f.shape[0]):
            cand = (R(0) - f[i]) / fneq[i]
            m = np.where(((f[i] < 0) | (fneq[i] < 0)) & (cand < m), cand, m)
    return m


def newton(grid, f, fneq, alpha0, entropy_tol, alpha_tol, log2=False):
    """EstimateAlphaFromEntropy on the columns of f, fneq.  Returns (alpha, ok, steps); ok False: the reference's die()."""
    R = f.dtype.type
    _, _, nlw = _grid_tables(grid, R)
    etol, atol, a11 = R(entropy_tol), R(alpha_tol), R(1.1)
    ent = entropy(grid, f, log2)
    amax = max_alpha(f, fneq)
    alpha = np.array(alpha0, dtype=f.dtype).copy()
    n = alpha.shape[0]
    steps = np.zeros(n, dtype=np.int64)
    done = np.zeros(n, dtype=bool)
    fail = np.zeros(n, dtype=bool)
    with np.errstate(all='ignore'):
        for _ in range(2002):
            if done.all():
                break
            ent_ineq = np.zeros_like(alpha)
            dent = np.zeros_like(alpha)
            for i in range(grid.Q):
                t = f[i] + alpha * fneq[i]
                h = _ln(t, log2) + nlw[i]
                ent_ineq = ent_ineq + t * h
                dent = dent + fneq[i] * (h + R(1))
            act = ~done
            restart = act & np.isnan(ent_ineq) & (alpha != a11)
            alpha = np.where(restart, a11, alpha)
            act &= ~restart
            inc = ent_ineq - ent
            done |= act & (np.abs(inc) < etol)
            act &= ~done
            new = alpha - inc / dent
            new = np.where(new > amax, R(0.5) * (alpha + amax), new)
            done |= act & (np.abs(new - alpha) < atol)
            act &= ~done
            giveup = act & np.isnan(new) & (alpha == a11)
            fail |= giveup
            done |= giveup
            act &= ~done
            alpha = np.where(act, new, alpha)
            steps += act
            over = act & (steps > 1000)
            fail |= over
            done |= over
    fail |= (alpha < R(1)) | ~np.isfinite(alpha)
    return alpha, ~fail, steps


def beta_of(visc, R):
    """1 / (2 tau0 + 1), tau0 = visc / cs^2, in precision R (slf_sweep.h make_params)."""
    return R(1) / (R(2) * R(3.0 * visc) + R(1))


def default_entropy_tolerance(dtype):
    return 1e-6 if np.dtype(dtype) == np.float32 else 1e-10


def collide(grid, f, visc, alpha_start=None, entropic_eq=False, incompressible=False, entropy_tol=None, alpha_tol=1e-10,
            log2=False):
    """One entropic collision of the columns of f [Q, n].  alpha_start: the Newton start values (None: 2).
    Returns dict(f=post-collision populations, alpha, ok, dev, regime (0 / 1 / 2), rho, v, fneq)."""
    f = np.asarray(f)
    R = f.dtype.type
    if entropy_tol is None:
        entropy_tol = default_entropy_tolerance(f.dtype)
    rho, v = macros(grid, f, incompressible)
    with np.errstate(all='ignore'):
        fe = feq_entropic(grid, rho, v) if entropic_eq else feq_bgk(grid, rho, v, incompressible)
        fneq = fe - f
    dev, a = a_coeffs(f, fneq)
    n = f.shape[1]
    alpha = np.full(n, R(2), dtype=f.dtype)
    ok = np.ones(n, dtype=bool)
    with np.errstate(all='ignore'):
        nw = dev >= R(0.01)           # (dev is never a NaN: the max() ignores one)
        ser = ~nw & (dev >= R(1e-6))
        if ser.any():
            alpha[ser] = _series_from_raw([x[ser] for x in a])
        if nw.any():
            start = np.full(n, R(2), dtype=f.dtype) if alpha_start is None else np.asarray(alpha_start, dtype=f.dtype)
            al, good, _ = newton(grid, f[:, nw], fneq[:, nw], start[nw], entropy_tol, alpha_tol, log2)
            alpha[nw] = al
            ok[nw] = good
        ab = alpha * beta_of(visc, R)
        post = np.where(ok[None, :], f + ab[None, :] * fneq, f)
    regime = np.where(nw, 2, np.where(ser, 1, 0))
    return dict(f=post, alpha=alpha, ok=ok, dev=dev, regime=regime, rho=rho, v=v, fneq=fneq)


class ElbmTwin(object):
    """A periodic box [Q, (nz,) ny, nx]; wall[...] True: full-way bounce-back node (no collision, populations reversed),
    everything else fluid.  step(): collide, then stream with periodic wrap.  The alpha field is kept when `alpha_field`
    (warm start); nodes whose solver gave up keep their populations and alpha and are counted in `failed`."""

    def __init__(self, grid, f, visc, wall=None, alpha_field=True, **kw):
        self.grid, self.visc, self.kw = grid, visc, kw
        self.f = np.array(f)
        self.shape = self.f.shape[1:]
        self.wall = np.zeros(self.shape, dtype=bool) if wall is None else np.asarray(wall, dtype=bool)
        self.alpha = np.full(self.shape, 2.0, dtype=self.f.dtype) if alpha_field else None
        self.failed = 0
        self.regime_counts = np.zeros(3, dtype=np.int64)

    @classmethod
    def from_fields(cls, grid, rho, v, visc, dtype=np.float64, **kw):
        """Initial populations = the BGK equilibrium of (rho, v), as SetInitialConditions."""
        rho = np.asarray(rho, dtype=dtype)
        vv = [np.asarray(c, dtype=dtype) for c in v] + [np.zeros_like(rho)] * (3 - len(v))
        return cls(grid, feq_bgk(grid, rho, vv), visc, **kw)

    def step(self):
        g, Q = self.grid, self.grid.Q
        fluid = ~self.wall
        cols = self.f[:, fluid]
        r = collide(g, cols, self.visc, alpha_start=None if self.alpha is None else self.alpha[fluid], **self.kw)
        self.failed += int((~r['ok']).sum())
        self.regime_counts += np.bincount(r['regime'], minlength=3)
        post = self.f.copy()
        post[:, fluid] = r['f']
        if self.alpha is not None:
            self.alpha[fluid] = np.where(r['ok'], r['alpha'], self.alpha[fluid])
        if self.wall.any():
            w = self.f[:, self.wall]
            post[:, self.wall] = w[g.idx_opposite]
        nd = len(self.shape)
        for i in range(Q):
            e = g.basis[i]
            shift = tuple(e[nd - 1 - ax] for ax in range(nd))       # array axes are (z,) y, x
            self.f[i] = np.roll(post[i], shift, axis=tuple(range(nd)))

    def run(self, n):
        for _ in range(n):
            self.step()
        return self

    def macros(self):
        rho, v = macros(self.grid, self.f.reshape(self.grid.Q, -1))
        return rho.reshape(self.shape), [c.reshape(self.shape) for c in v[:self.grid.dim]]
