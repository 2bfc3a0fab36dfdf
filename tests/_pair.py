"""BoxSim (the HIP kernels) and OracleBox (the CPU oracle) on the same inputs, and what separates their results
(test-only helper)."""
import numpy as np

from sailfish_amd.box import BoxSim, make_box_desc
from tests._oracle_box import OracleBox, synthetic_fields


def run_pair(backend, grid, size, steps, periodic, node_map_fn=None, u_scale=0.05, init='synthetic', sims=False, **kw):
    """init: 'synthetic' (tests/_oracle_box.synthetic_fields), 'rest', or the fields themselves as (rho, [v...]).
    sims = True: returns (result, BoxSim, OracleBox) for whoever wants to look at more than the error figures."""
    desc = make_box_desc(grid, size, **kw)
    nmap = node_map_fn(desc) if node_map_fn else None
    if isinstance(init, tuple):
        rho, v = init
    else:
        rho, v = synthetic_fields(size, grid.dim)
        if init == 'rest':
            rho = np.ones_like(rho)
            v = [np.zeros_like(c) for c in v]
    pair = []
    for cls, args in ((BoxSim, (backend, desc)), (OracleBox, (desc,))):
        s = cls(*args, periodic=periodic, node_map=nmap)
        s.set_fields(rho, v)
        s.initial_conditions()
        s.run(steps, save_last=True)
        pair.append(s)
    g, o = pair
    g_rho, g_v = g.fetch_fields()
    f_g = g.real_view(g.get_dist())
    f_o = o.real_view(o.current_dist())
    res = {'dist_exact': np.array_equal(f_g, f_o, equal_nan=True)}
    r_g, r_o = g.real_view(g_rho), o.real_view(o.rho)
    mask = np.isfinite(r_o)
    assert np.array_equal(mask, np.isfinite(r_g))
    res['rho_err'] = float(np.max(np.abs(r_g[mask] - r_o[mask]) / np.abs(r_o[mask])))
    verr = 0.0
    for d in range(grid.dim):
        a, b = g.real_view(g_v[d])[mask], o.real_view(o.v[d])[mask]
        verr = max(verr, float(np.max(np.abs(a - b))) / u_scale)
    res['v_err'] = verr
    fm = np.isfinite(f_o)
    res['dist_err'] = float(np.max(np.abs(f_g[fm] - f_o[fm])))
    if sims:
        return res, g, o
    return res
