"""Host side of NTWallTMS (no GPU): the node type's kernel kind, what a subdomain with TMS walls encodes to, the module
descriptor the runner fills in, and what is refused."""
import numpy as np
import pytest

from sailfish_amd import hipabi, lb_base, lb_single
from sailfish_amd import node_type as nt
from sailfish_amd.subdomain import Subdomain2D, Subdomain3D
from tests import _host
from tests.test_elbm_host import RecordingBackend


class _Channel2D(Subdomain2D):
    def boundary_conditions(self, hx, hy):
        self.set_node((hy == 0) | (hy == self.gy - 1), nt.NTWallTMS)

    def initial_conditions(self, sim, hx, hy):
        sim.rho[:] = 1.0


class _Channel3D(Subdomain3D):
    def boundary_conditions(self, hx, hy, hz):
        self.set_node((hx == 0) | (hx == self.gx - 1), nt.NTWallTMS)

    def initial_conditions(self, sim, hx, hy, hz):
        sim.rho[:] = 1.0


class _Sim2D(lb_single.LBFluidSim, lb_base.LBForcedSim):
    subdomain = _Channel2D


class _Sim3D(lb_single.LBFluidSim, lb_base.LBForcedSim):
    subdomain = _Channel3D


class _ShanChen2D(lb_single.LBSingleFluidShanChen):
    subdomain = _Channel2D


def _runner(sim_cls, dim, **kw):
    cfg_kw = dict(lat_nx=12, lat_ny=10, precision='double', periodic_x=True)
    if dim == 3:
        cfg_kw.update(lat_nz=6, periodic_x=False, periodic_y=True, periodic_z=True)
    cfg_kw.update(kw)
    cfg, specs, runners = _host.build_runners(sim_cls, dim, None, cfg_kw, backend_factory=RecordingBackend)
    return cfg, runners[0]


def test_kind_table():
    assert hipabi.SLF_NK_WALL_TMS == 16
    assert nt.HIP_KIND[nt.NTWallTMS] == hipabi.SLF_NK_WALL_TMS
    assert nt.hip_kind(nt.NTWallTMS, 'AA') == nt.hip_kind(nt.NTWallTMS, 'AB') == hipabi.SLF_NK_WALL_TMS
    # the flags are the reference's: a wet node with standard macroscopic fields and link tags, half a node from the wall
    t = nt.NTWallTMS
    assert (t.wet_node, t.standard_macro, t.link_tags, t.needs_orientation, t.allow_unused, t.location) == \
        (True, True, True, True, True, 0.5)
    assert t.id in nt.get_wet_node_type_ids() and t.id in nt.get_link_tag_node_type_ids()
    assert hipabi.SLF_NK_WALL_TMS in lb_single.LBFluidSim.ROUNDOFF_KINDS


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('dim', [2, 3])
def test_subdomain_with_tms_walls_encodes(dim, pattern):
    cfg, r = _runner(_Sim2D if dim == 2 else _Sim3D, dim, access_pattern=pattern)
    r.prepare()
    desc = r.backend.desc
    kinds = list(desc.type_kind[:desc.n_types])
    assert hipabi.SLF_NK_WALL_TMS in kinds and hipabi.SLF_NK_HALF_BB not in kinds
    assert desc.use_link_tags == 1                       # a TMS-only geometry turns the link tags on
    enc = r._subdomain._encoder
    dense = enc._type_id_remap[nt.NTWallTMS.id]
    assert kinds[dense] == hipabi.SLF_NK_WALL_TMS
    # the wall nodes carry tags: some links of every wall node point to wet nodes, some do not
    node_map = np.asarray(r._subdomain.encoded_map())
    shift = enc._bits_type + enc._bits_param + enc._bits_scratch
    wall = (node_map & ((1 << enc._bits_type) - 1)) == dense
    tags = (node_map >> shift)[wall]
    full = (1 << (r._sim.grid.Q - 1)) - 1
    assert wall.any() and np.all(tags != 0) and np.all(tags != full)


def test_roundoff_accepts_tms_and_names_what_it_refuses():
    kw = dict(incompressible=hipabi.SLF_DENSITY_ROUNDOFF,
              type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_GHOST, hipabi.SLF_NK_WALL_TMS])
    lb_single.LBFluidSim.check_module_desc(kw)
    cfg, r = _runner(_Sim3D, 3, access_pattern='AA', minimize_roundoff=True)
    r.prepare()
    assert r.backend.desc.incompressible == hipabi.SLF_DENSITY_ROUNDOFF


def test_shan_chen_with_tms_is_refused():
    kw = dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_SINGLE, type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_WALL_TMS])
    with pytest.raises(NotImplementedError, match='NTWallTMS'):
        lb_single.LBSingleFluidShanChen.check_module_desc(kw)
    with pytest.raises(NotImplementedError, match='NTWallTMS'):
        lb_base.LBSim.check_module_desc(dict(kw, simtype=hipabi.SLF_SIM_SHAN_CHEN_BINARY))
    cfg, r = _runner(_ShanChen2D, 2, G=1.0, sc_potential='linear')
    with pytest.raises(NotImplementedError, match='NTWallTMS'):
        r.prepare()
