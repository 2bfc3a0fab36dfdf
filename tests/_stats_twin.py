"""numpy restatement of the two statistics kernels (sailfish_amd/csrc/slf_stats.hip): the stencil and v_sq in the
field's precision and in the kernel's operation order, the 22 profile terms in double in the kernel's order.  What the
kernels ADD is therefore the twin's terms bit for bit; only the order of addition differs, which `sum_bound` covers.
Arrays are [nz, ny, nx] over the real nodes (no ghost layer)."""
import math

import numpy as np

PROFILE_KEYS = tuple('%s_m%d' % (f, m) for f in ('ux', 'uy', 'uz', 'rho') for m in range(1, 5)) + \
    ('ux_uy', 'ux_uz', 'uy_uz', 'ux_rho', 'uy_rho', 'uz_rho')
U = 2.0 ** -53          # unit round-off of double


def kida(size, max_v=0.05, dtype=np.float64, shift=(0, 0, 0)):
    """The Kida field on a box of size = (nx, ny, nz), formed in double and rounded to dtype: [3, nz, ny, nx]."""
    nx, ny, nz = size
    hz, hy, hx = np.mgrid[0:nz, 0:ny, 0:nx]
    x = (hx + shift[0]) * np.pi * 2.0 / nx
    y = (hy + shift[1]) * np.pi * 2.0 / ny
    z = (hz + shift[2]) * np.pi * 2.0 / nz
    sin, cos = np.sin, np.cos
    v = np.zeros((3, nz, ny, nx), dtype=dtype)
    v[0] = max_v * sin(x) * (cos(3 * y) * cos(z) - cos(y) * cos(3 * z))
    v[1] = max_v * sin(y) * (cos(3 * z) * cos(x) - cos(z) * cos(3 * x))
    v[2] = max_v * sin(z) * (cos(3 * x) * cos(y) - cos(x) * cos(3 * y))
    return v


def diff(f, axis):
    """(f[+1] - f[-1]) 0.5 inside, f[+1] - f on the first and f - f[-1] on the last layer of `axis`, in f's precision."""
    assert f.shape[axis] >= 2
    half = f.dtype.type(0.5)

    def at(s):
        return tuple(s if a == axis else slice(None) for a in range(f.ndim))
    out = np.empty_like(f)
    out[at(slice(1, -1))] = (f[at(slice(2, None))] - f[at(slice(None, -2))]) * half
    out[at(slice(0, 1))] = f[at(slice(1, 2))] - f[at(slice(0, 1))]
    out[at(slice(-1, None))] = f[at(slice(-1, None))] - f[at(slice(-2, -1))]
    return out


def vorticity(v):
    """[3, nz, ny, nx]: (duz/dy - duy/dz, dux/dz - duz/dx, duy/dx - dux/dy); array axes are (z, y, x)."""
    vx, vy, vz = v[0], v[1], v[2]
    return np.array((diff(vz, 1) - diff(vy, 0), diff(vx, 0) - diff(vz, 2), diff(vy, 2) - diff(vx, 1)))


def ke_fields(v, excluded=None):
    """v_sq = (vx vx + vy vy) + vz vz and vort_sq = (wx wx + wy wy) + wz wz in v's precision; 0 where `excluded`."""
    vx, vy, vz = v[0], v[1], v[2]
    v_sq = (vx * vx + vy * vy) + vz * vz
    w = vorticity(v)
    vort_sq = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    assert v_sq.dtype == v.dtype and vort_sq.dtype == v.dtype
    if excluded is not None:
        v_sq[excluded] = 0
        vort_sq[excluded] = 0
    return v_sq, vort_sq


def profile_terms(v, rho):
    """[22, nz, ny, nx] double: the field value converted to double, powers multiplied left to right, a correlation one
    product (the reference's _compute_stats)."""
    f = [np.asarray(a, dtype=np.float64) for a in (v[0], v[1], v[2], rho)]
    t = []
    for a in f:
        p2 = a * a
        p3 = p2 * a
        p4 = p3 * a
        t += [a, p2, p3, p4]
    t += [f[0] * f[1], f[0] * f[2], f[1] * f[2], f[0] * f[3], f[1] * f[3], f[2] * f[3]]
    return np.array(t)


def sum_and_bound(terms, divisions=0, divisor=1.0):
    """(fsum(terms) / divisor, bound): a sum of n double terms added in ANY order is within n 2^-53 sum|t| of the exact
    sum; each division that follows adds |result| 2^-53."""
    t = np.asarray(terms, dtype=np.float64).ravel()
    exact = math.fsum(t)
    bound = t.size * U * math.fsum(np.abs(t))
    res = exact / divisor
    return res, bound / abs(divisor) + divisions * abs(res) * U


def profiles(terms, axis):
    """axis 0 / 1 / 2 = x / y / z.  ([22, n] fsum of the terms over the two other axes, [22, n] bounds)."""
    arr_axis = 3 - axis                 # terms is [22, z, y, x]
    moved = np.moveaxis(terms, arr_axis, 1)
    n = moved.shape[1]
    ref = np.zeros((terms.shape[0], n))
    bound = np.zeros_like(ref)
    for k in range(terms.shape[0]):
        for p in range(n):
            ref[k, p], bound[k, p] = sum_and_bound(moved[k, p])
    return ref, bound
