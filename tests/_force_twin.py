"""Numpy twin of the momentum-exchange force (sailfish_amd/csrc/slf_force.hip; reference ForceObject, lb_base.py:418-456
with subdomain.py:734-770 and subdomain_runner.py:1459-1526).  Test-only.  Two levels:

  * table level -- link_terms() / fsum_force() / bound(): what the kernel is asked to compute from (dist, idx, idx2, dirs),
    with the per-link bracket formed in the module's precision, the terms exact in double and the sums by math.fsum;
  * geometry level -- box_links() / post_propagation_real() / force_on_box(): the force from the MEANING of the arrays, written
    without the runner's index tables: the links are found on the node map, and the post-propagation value of direction k
    at node x is read where the access pattern keeps it (in-place pattern after an odd number of steps: slot opp(k) at
    x - e_k).  That the runner's one table serves both patterns and both parities is what the tests compare this against.
"""
import math

import numpy as np


def basis3(grid):
    """[Q, 3] integer array of the lattice vectors, z = 0 in 2-D."""
    e = np.zeros((grid.Q, 3), dtype=np.int64)
    e[:, :grid.dim] = np.array(grid.basis, dtype=np.int64)
    return e


def link_terms(dist_flat, idx, idx2, dirs, grid):
    """[n, 3] float64: (double)(dist[idx] + dist[idx2]) * e_opp(dirs), the bracket in dist_flat's precision."""
    m = (dist_flat[np.asarray(idx, dtype=np.int64)] + dist_flat[np.asarray(idx2, dtype=np.int64)]).astype(np.float64)
    e = basis3(grid)[np.array(grid.idx_opposite)[np.asarray(dirs, dtype=np.int64)]].astype(np.float64)
    return m[:, None] * e


def fsum_force(terms):
    return [math.fsum(terms[:, k]) for k in range(3)]


def bound(terms):
    """Error bound of any order of summation of n terms in double (tests/test_gpu_stats.py): n 2^-53 sum |t|, per component."""
    n = terms.shape[0]
    return [n * 2.0 ** -53 * math.fsum(np.abs(terms[:, k])) for k in range(3)]


def box_links(vis_map, location, start, end, grid):
    """Links of the box start .. end (global coordinates, inclusive) on the real-node type map `vis_map` (numpy axis order)
    of a subdomain at `location`: (dirs, solid, fluid) with solid / fluid integer arrays [n, dim] of real-node coordinates
    in numpy axis order; ascending direction, then np.where order.  The neighbourhood wraps around the map."""
    dim = grid.dim
    grids = np.indices(vis_map.shape)
    cond = vis_map != 0
    for axis in range(dim):
        g = grids[dim - 1 - axis] + location[axis]
        cond &= (g >= start[axis]) & (g <= end[axis])
    dirs, solid, fluid = [], [], []
    shape = np.array(vis_map.shape)
    for i, vec in enumerate(grid.basis[1:], 1):
        step = np.array([int(c) for c in reversed(vec)])
        s = np.argwhere(cond)
        f = (s + step) % shape
        hit = vis_map[tuple(f.T)] == 0
        dirs.append(np.full(int(hit.sum()), i, dtype=np.int64))
        solid.append(s[hit])
        fluid.append(f[hit])
    return np.concatenate(dirs), np.concatenate(solid), np.concatenate(fluid)


def post_propagation_real(real, k, pos, grid, in_place_odd):
    """Post-propagation value of direction k at the real nodes `pos` ([n, dim], numpy axis order) of the real-node array
    real[Q, (nz,) ny, nx] (periodic axes wrap onto real nodes).  in_place_odd: in-place pattern after an odd number of
    steps."""
    if not in_place_odd:
        return real[(k,) + tuple(pos.T)]
    step = np.array([int(c) for c in reversed(grid.basis[k])])
    src = (pos - step) % np.array(real.shape[1:])
    return real[(grid.idx_opposite[k],) + tuple(src.T)]


def force_terms_on_box(real, vis_map, location, start, end, grid, in_place_odd):
    """[n, 3] float64 terms of the force on the box from the real-node populations real[Q, ...]."""
    dirs, solid, fluid = box_links(vis_map, location, start, end, grid)
    e = basis3(grid)
    opp = np.array(grid.idx_opposite)
    terms = np.zeros((len(dirs), 3), dtype=np.float64)
    for i in np.unique(dirs):
        sel = dirs == i
        a = post_propagation_real(real, int(opp[i]), solid[sel], grid, in_place_odd)
        b = post_propagation_real(real, int(i), fluid[sel], grid, in_place_odd)
        m = (a + b) if not in_place_odd else (b + a)          # (the kernel's operand order; the sum is commutative)
        terms[sel] = m.astype(np.float64)[:, None] * e[opp[i]].astype(np.float64)
    return terms


def force_on_box(real, vis_map, location, start, end, grid, in_place_odd):
    return fsum_force(force_terms_on_box(real, vis_map, location, start, end, grid, in_place_odd))
