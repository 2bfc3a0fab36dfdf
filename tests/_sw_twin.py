"""numpy twin of the shallow-water model (slf_module_desc::equilibrium = SLF_EQ_SHALLOW_WATER, LBFreeSurface): what the SW
instantiations of the per-node sweep (csrc/slf_kernels.hip) and of SetInitialConditions compute on D2Q9.

Every floating-point operation is one numpy operation in the module's format, in the order of csrc/slf_node.h
(sw_equilibrium, bgk_relax_accel<..., SW>); the kernels are built with -ffp-contract=off, so they have nothing to round
differently.  The equilibrium, h the depth, g the gravity:

    gh15 = (1.5 g) h                    u15 = 1.5 (vx vx + vy vy)
    fe_i = w_i (h ((gh15 + eu (3 + 4.5 eu)) - u15))        i = 1 .. 8, eu = e_i . v
    fe_0 = h - (((fe_1 + fe_2) + fe_3) + ... + fe_8)         LAST: the populations sum to h

The collision is tests/_lat_twin.relax with this equilibrium in the polynomial's place -- once in the relaxation, twice in
the exact-difference force; moments, the Guo term, the velocity shift, bounce-back, the half-way store and streaming are
those of every single-fluid module (tests/_accf_twin.AccfTwin.step), and the slip reflection moves populations without
arithmetic.  sw_rest_reference() is the rest population the REFERENCE relaxes to, kept for the tests that show what it
does to the mass.

SwTwin has the interface of oracle.OracleSim (new_dist, new_field, init, step, pbc, sparse); SwTwinBox is the step
sequence of sailfish_amd.box.BoxSim on it.  model(): the bare periodic box the issue's numbers were measured on.
Test-only."""
import numpy as np

from oracle.oracle import OracleSim
from sailfish_amd import hipabi, sym
from tests import _lat_twin as lt
from tests._accf_twin import AccfTwin
from tests._oracle_box import OracleBox

PROP_AB, PROP_AA_EVEN, PROP_AA_ODD = lt.PROP_AB, lt.PROP_AA_EVEN, lt.PROP_AA_ODD
GRID = sym.D2Q9


def sw_equilibrium(h, v, g, R, rest=None):
    """[9, n] in the format R; h: [n], v: two [n] arrays, g: scalar.  rest: a function (h, v, g, R, moving) for another
    rest population (sw_rest_reference)."""
    w = lt.weights(GRID, R)
    gh15 = (R(1.5) * R(g)) * h
    u15 = lt.usq15(v, R)
    fe = [None] * 9
    for i in range(1, 9):
        eu = lt.edot(GRID, i, v, h)
        fe[i] = w[i] * (h * ((gh15 + eu * (R(3) + R(4.5) * eu)) - u15))
    if rest is not None:
        fe[0] = rest(h, v, g, R, fe[1:])
    else:
        s = fe[1]
        for i in range(2, 9):
            s = s + fe[i]
        fe[0] = h - s
    return np.stack(fe)


def sw_rest_reference(h, v, g, R, moving=None):
    """The reference's rest population (sym_equilibrium.py:80-81): h - w_0 h (15/8 g h - 3 v^2).  NOT what the kernels
    compute: it exceeds the conserving one by 2 h v^2."""
    w0 = lt.weights(GRID, R)[0]
    vsq = v[0] * v[0] + v[1] * v[1]
    return h - w0 * h * (R(1.875) * R(g) * h - R(3) * vsq)


def sw_relax(f, h, v, omega, guo_pref, accel, edm, g, R, rest=None):
    """bgk_relax_accel<L, R, SW = true>: the post-collision populations and the velocity the sweep stores."""
    if accel is not None and edm:
        vs = [c + a for c, a in zip(v, accel)]
        fe = sw_equilibrium(h, v, g, R, rest)
        fs = sw_equilibrium(h, vs, g, R, rest)
        out = [(f[i] + omega * (fe[i] - f[i])) + (fs[i] - fe[i]) for i in range(9)]
        return np.stack(out), [c + R(0.5) * a for c, a in zip(v, accel)]
    if accel is not None:
        v = [c + R(0.5) * a for c, a in zip(v, accel)]
    fe = sw_equilibrium(h, v, g, R, rest)
    out = [f[i] + omega * (fe[i] - f[i]) for i in range(9)]
    if accel is not None:
        # the Guo term of tests/_lat_twin.relax, which reads rho = h and the shifted velocity
        guo = lt.guo_term(GRID, h, v, [np.zeros_like(h) + a for a in accel], guo_pref, R)
        out = [out[i] + guo[i] for i in range(9)]
    return np.stack(out), v


def slip_image(i, orientation):
    """The direction whose normal component (along the axis of `orientation`, 1..4) is reversed; i itself without one."""
    n = GRID.basis[GRID.dir2vecidx[orientation]]
    e = GRID.basis[i]
    if sum(a * b for a, b in zip(e, n)) == 0:
        return i
    img = tuple(-a if b else a for a, b in zip(e, n))
    return [tuple(x) for x in GRID.basis].index(img)


class SwTwin(AccfTwin):
    """One subdomain of a shallow-water module; node kinds fluid, ghost, unused, propagation-only, full-way and half-way
    bounce-back, slip.  rest: another rest population for the collision and the initial state (sw_rest_reference)."""

    def __init__(self, desc, rest=None, R=None):
        assert desc.lattice == hipabi.SLF_D2Q9 and int(desc.equilibrium) == hipabi.SLF_EQ_SHALLOW_WATER and desc.gravity > 0
        assert not int(desc.incompressible)
        AccfTwin.__init__(self, desc)
        self.rest = rest
        if R is not None:           # the same module in another format (the wider one the tolerances are sized with):
            self.R = self.dtype = R      # step() on arrays of that format; init / pbc / sparse stay the descriptor's

    def init(self, dist, rho, vx, vy, vz=None):
        R = self.R
        sl = tuple(slice(0, n) for n in self.lat)
        with np.errstate(all='ignore'):
            fe = sw_equilibrium(rho[sl].astype(R), [vx[sl].astype(R), vy[sl].astype(R)], self.desc.gravity, R, self.rest)
        dist[(slice(None),) + sl] = fe

    def step(self, prop, nmap, din, dout, rho, vx, vy, vz=None, options=0, region=None):
        d, R, opp = self.desc, self.R, self.opp
        z, y, x = self.zyx
        rows = np.ones(len(y), dtype=bool) if region is None else (y >= region[0]) & (y < region[1])
        here = (z, y, x)
        if d.fluid_only:
            code = np.zeros(len(z), dtype=np.uint32)
            kind = np.full(len(z), hipabi.SLF_NK_FLUID)
        else:
            code = nmap[here]
            kind = np.array(list(d.type_kind[:d.n_types]))[code & np.uint32(d.nt_type_mask)]
        assert np.isin(kind, lt.EXCLUDED + lt.WET + (hipabi.SLF_NK_FULL_BB, hipabi.SLF_NK_SLIP)).all()
        active = ~np.isin(kind, lt.EXCLUDED) & rows
        wet = np.isin(kind, lt.WET) & active
        fwd, bwd = self._neighbour(+1), self._neighbour(-1)
        if prop == PROP_AA_ODD:
            f = np.stack([din[(opp[i],) + bwd[i]] for i in range(9)])
        else:
            f = np.stack([din[(i,) + here] for i in range(9)])
        omega = R(1.0 / d.tau)
        guo_pref = R(3.0 * (1.0 - 0.5 / d.tau))
        wet_at = tuple(c[wet] for c in here)
        accel = self.node_accel(wet_at)
        if accel is not None:
            accel = accel[:2]
        edm = int(d.force_implementation) == hipabi.SLF_FORCE_EDM
        fw = f[:, wet]
        with np.errstate(all='ignore'):
            h, v = lt.macro(GRID, fw, False, R)
            if d.relaxation_enabled:
                fw, v = sw_relax(fw, h, v, omega, guo_pref, accel, edm, d.gravity, R, self.rest)
        f[:, wet] = fw
        if options & 1:
            rho[wet_at] = h
            vx[wet_at], vy[wet_at] = v
        orient_shift = d.nt_misc_shift + d.nt_param_shift + d.nt_scratch_shift
        orientation = code >> np.uint32(orient_shift)
        bb = (kind == hipabi.SLF_NK_FULL_BB) & rows
        f[:, bb] = f[opp][:, bb]
        for o in range(1, 5):
            m = (kind == hipabi.SLF_NK_SLIP) & (orientation == o) & rows
            if m.any():
                f[:, m] = f[[slip_image(i, o) for i in range(9)]][:, m]
        hb = (kind == hipabi.SLF_NK_HALF_BB) & active
        if hb.any():
            assert d.use_link_tags
            for i in range(1, 9):
                m = hb & (((orientation >> np.uint32(i - 1)) & np.uint32(1)) == 0)
                if not m.any():
                    continue
                if prop == PROP_AA_EVEN:
                    dout[(i,) + tuple(c[m] for c in fwd[i])] = f[i, m]
                else:
                    dout[(opp[i],) + tuple(c[m] for c in here)] = f[i, m]
        for i in range(9):
            if prop == PROP_AA_EVEN:
                dout[(opp[i],) + tuple(c[active] for c in here)] = f[i, active]
            else:
                dout[(i,) + tuple(c[active] for c in fwd[i])] = f[i, active]


class SwTwinBox(OracleBox):
    """tests/_oracle_box.OracleBox with the twin in the oracle's place (accel_field as in tests/_accf_twin.AccfTwinBox)."""

    def __init__(self, desc, periodic=(False, False, False), node_map=None, accel_field=None, fill=np.nan, rest=None):
        super(SwTwinBox, self).__init__(desc, periodic, node_map)
        self.o = SwTwin(desc, rest)
        self.accel_field = None
        if accel_field is not None:
            self.accel_field = np.full((self.dim,) + self.shape, fill, dtype=self.dtype)
            for k in range(self.dim):
                self.real_view(self.accel_field[k])[...] = np.asarray(accel_field[k], dtype=np.float64)
            self.o.set_accel_field(self.accel_field)


def wider(dtype):
    """The next wider format, or None where long double is no wider than double."""
    if dtype is np.float32:
        return np.float64
    return np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else None


# ---- the bare periodic box -------------------------------------------------------------------------------------------------

def model(nx, ny, g, visc, h, steps, R=np.float64, rest=None, v=None, record=None):
    """A fully periodic nx x ny box without ghost layers (np.roll), two-copy: `steps` collisions and streamings from the
    equilibrium of the depth h [ny, nx] (and the velocity v, default rest).  Returns the populations [9, ny, nx]; record(t, f)
    is called with the populations before every step."""
    h = np.asarray(h, dtype=R)
    v = [np.zeros_like(h), np.zeros_like(h)] if v is None else [np.asarray(c, dtype=R) for c in v]
    omega = R(1.0 / sym.relaxation_time(visc))
    shape = h.shape
    f = sw_equilibrium(h.ravel(), [c.ravel() for c in v], g, R, rest).reshape((9,) + shape)
    for t in range(steps):
        if record is not None:
            record(t, f)
        flat = f.reshape(9, -1)
        hh, vv = lt.macro(GRID, flat, False, R)
        post, _ = sw_relax(flat, hh, vv, omega, R(0), None, False, g, R, rest)
        post = post.reshape((9,) + shape)
        f = np.stack([np.roll(post[i], (GRID.basis[i][1], GRID.basis[i][0]), axis=(0, 1)) for i in range(9)])
    if record is not None:
        record(steps, f)
    return f


def period_from_crossings(signal):
    """The period of an oscillation about zero from its zero crossings (linear interpolation): twice the mean spacing."""
    s = np.asarray(signal, dtype=np.float64)
    k = np.nonzero(np.signbit(s[:-1]) != np.signbit(s[1:]))[0]
    assert len(k) >= 3, 'fewer than three zero crossings'
    t = k + s[k] / (s[k] - s[k + 1])
    return 2.0 * (t[-1] - t[0]) / (len(t) - 1)
