"""Host side of --model=elbm (no GPU): options, module descriptor, the alpha field of LBEntropicFluidSim, the argument
list of the kernel call, what is refused, and the alpha field's way through a checkpoint."""
import argparse
import ctypes
import os

import numpy as np
import pytest

from sailfish_amd import hipabi, lb_base, lb_single, sym
from sailfish_amd import node_type as nt
from sailfish_amd.box import make_box_desc
from sailfish_amd.subdomain import Subdomain2D
from tests import _host
from tests._oracle_backend import OracleBackend


def _parse(argv):
    p = argparse.ArgumentParser()
    lb_single.LBFluidSim.add_options(p, 2)
    return p.parse_args(argv)


def test_options_and_defaults():
    o = _parse([])
    assert (o.model, o.entropic_equilibrium, o.entropy_tolerance, o.alpha_tolerance) == ('bgk', False, 0.0, 1e-10)
    o = _parse(['--model=elbm', '--entropic_equilibrium', '--entropy_tolerance=1e-8', '--alpha_tolerance=1e-7'])
    assert (o.model, o.entropic_equilibrium, o.entropy_tolerance, o.alpha_tolerance) == ('elbm', True, 1e-8, 1e-7)
    with pytest.raises(SystemExit):
        _parse(['--model=cumulant'])


def test_tau0_and_descriptor_fields():
    assert lb_single.LBFluidSim.elbm_tau0(sym.D2Q9, 0.02) == pytest.approx(0.06)
    for grid in (sym.D2Q9, sym.D3Q19):
        assert grid.model_supported('elbm')
        assert [float(w) for w in grid.entropic_weights] == [float(w) for w in grid.weights]
    d = lb_single.LBFluidSim.elbm_desc(sym.D3Q19, 0.01, 'single')
    assert d['model'] == hipabi.SLF_ELBM == 2 and d['entropy_tolerance'] == 1e-6 and d['alpha_tolerance'] == 1e-10
    assert d['entropic_equilibrium'] == 0 and not any(d['mrt_rates'])
    assert lb_single.LBFluidSim.elbm_desc(sym.D3Q19, 0.01, 'double')['entropy_tolerance'] == 1e-10
    assert lb_single.LBFluidSim.elbm_desc(sym.D2Q9, 0.01, 'double', True, 3e-9, 1e-8) == dict(
        model=2, mrt_rates=[0.0] * 9, entropic_equilibrium=1, entropy_tolerance=3e-9, alpha_tolerance=1e-8)
    # the new fields sit at the END of slf_module_desc
    names = [f[0] for f in hipabi.SlfModuleDesc._fields_]
    assert names[-3:] == ['entropic_equilibrium', 'entropy_tolerance', 'alpha_tolerance']
    desc = make_box_desc(sym.D2Q9, (8, 8), model='elbm', precision='double', entropic_equilibrium=True)
    assert (desc.model, desc.entropic_equilibrium, desc.entropy_tolerance, desc.alpha_tolerance) == (2, 1, 1e-10, 1e-10)
    assert desc.struct_size == ctypes.sizeof(hipabi.SlfModuleDesc)
    assert make_box_desc(sym.D2Q9, (8, 8)).entropy_tolerance == 0.0          # bgk / mrt descriptors: as before


def test_entropic_sim_class():
    cls = lb_single.LBEntropicFluidSim
    fields = cls.fields()
    assert [(type(f), f.name) for f in fields] == [(lb_base.ScalarField, 'rho'), (lb_base.VectorField, 'v'),
                                                   (lb_base.ScalarField, 'alpha')]
    assert fields[2].init == 2.0 and cls.alpha_output and not lb_single.LBFluidSim.alpha_output
    cfg = _host.make_config(2)
    cls.modify_config(cfg)
    assert cfg.model == 'elbm'
    import sailfish.lb_single as alias           # the reference's import path
    assert alias.LBEntropicFluidSim is cls


class _Module(object):
    block_size = 64

    def __init__(self, desc):
        self.desc = desc


class RecordingBackend(OracleBackend):
    """Host memory as device memory; modules are their descriptors, kernels are recorded, nothing is launched."""

    def build(self, source):
        self.desc = source
        return _Module(source)

    def run_kernel(self, k, grid_size=None, stream=None):
        pass


class _Box(Subdomain2D):
    def boundary_conditions(self, hx, hy):
        self.set_node((hx == 0) | (hy == 0) | (hx == self.gx - 1), nt.NTFullBBWall)

    def initial_conditions(self, sim, hx, hy):
        sim.rho[:] = 1.0


class _EntropicSim(lb_single.LBEntropicFluidSim):
    subdomain = _Box


class _PlainElbmSim(lb_single.LBFluidSim):
    subdomain = _Box


class _ForcedSim(lb_single.LBFluidSim, lb_base.LBForcedSim):
    subdomain = _Box

    def __init__(self, config):
        super(_ForcedSim, self).__init__(config)
        self.add_body_force((1e-5, 0.0))


def _runner(sim_cls, tmp_path=None, **kw):
    cfg_kw = dict(lat_nx=24, lat_ny=16, precision='double')
    if tmp_path is not None:
        cfg_kw['checkpoint_file'] = os.path.join(str(tmp_path), 'cp')
    cfg_kw.update(kw)
    cfg, specs, runners = _host.build_runners(sim_cls, 2, None, cfg_kw, backend_factory=RecordingBackend)
    return cfg, runners[0]


@pytest.mark.parametrize('addressing', ['direct', 'indirect'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_kernel_call_signature(addressing, pattern):
    """(nodes,) map, dist_in, dist_out, rho, vx, vy, options, alpha: the alpha field is the LAST argument, behind the
    options word (reference lb_single.py:105-135)."""
    cfg, r = _runner(_EntropicSim, node_addressing=addressing, access_pattern=pattern, entropic_equilibrium=True)
    r.prepare()
    desc = r.backend.desc
    assert (desc.model, desc.entropic_equilibrium, desc.entropy_tolerance) == (hipabi.SLF_ELBM, 1, 1e-10)
    assert not any(desc.mrt_rates)
    lead = 1 if addressing == 'indirect' else 0
    sim = r._sim
    for pair in (r._kernels_none, r._kernels_full):
        for k in pair.primary + pair.secondary:
            assert k.name == 'CollideAndPropagate'
            assert k.fmt == 'P' * (lead + 6) + 'iP'
            assert k.args[-1] == r.gpu_field(sim.alpha) and k.args[lead + 3] == r.gpu_field(sim.rho)
            assert k.args[lead] == r.gpu_geo_map() and k.args[-2] in (0, 1, 2, 3)
            assert {k.args[lead + 1], k.args[lead + 2]} <= {r.gpu_dist(0, 0), r.gpu_dist(0, 1)}
    assert np.all(sim.alpha == 2.0)
    # without the class the model still runs, with no alpha array: the reference's signature
    cfg, r = _runner(_PlainElbmSim, model='elbm', access_pattern=pattern)
    r.prepare()
    assert r.backend.desc.model == hipabi.SLF_ELBM and r.backend.desc.entropic_equilibrium == 0
    assert r._kernels_none.primary[0].fmt == 'PPPPPPi'


def _kw(**over):
    kw = dict(model=hipabi.SLF_ELBM, mrt_rates=[0.0] * 9, incompressible=hipabi.SLF_DENSITY_COMPRESSIBLE,
              simtype=hipabi.SLF_SIM_LBM, entropic_equilibrium=0, type_kind=[hipabi.SLF_NK_FLUID])
    kw.update(over)
    return kw


REFUSALS = [
    (dict(mrt_rates=sym.mrt_rates(sym.D2Q9, 0.01)), 'MRT relaxation rates'),
    (dict(regularized=1), 'regularized / --subgrid'),
    (dict(subgrid=hipabi.SLF_SUBGRID_LES_SMAGORINSKY), 'regularized / --subgrid'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_SINGLE), 'single-fluid'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_BINARY), 'single-fluid'),
    (dict(incompressible=hipabi.SLF_DENSITY_ROUNDOFF), 'minimize_roundoff'),
    (dict(incompressible=hipabi.SLF_DENSITY_INCOMPRESSIBLE, entropic_equilibrium=1), '--incompressible'),
    (dict(has_force=1), 'body forces'),
    (dict(model=hipabi.SLF_BGK, entropic_equilibrium=1), 'entropic_equilibrium needs'),
]


@pytest.mark.parametrize('over,message', REFUSALS, ids=[m for _, m in REFUSALS])
def test_refusals(over, message):
    lb_single.LBFluidSim.check_module_desc(_kw())                                       # the plain module passes
    lb_single.LBFluidSim.check_module_desc(_kw(incompressible=hipabi.SLF_DENSITY_INCOMPRESSIBLE))
    with pytest.raises(NotImplementedError) as e:
        lb_single.LBFluidSim.check_module_desc(_kw(**over))
    assert message in str(e.value)


def test_refusals_through_the_runner():
    with pytest.raises(NotImplementedError, match='body forces'):
        _runner(_ForcedSim, model='elbm')[1].prepare()
    with pytest.raises(ValueError, match='needs --model=elbm'):
        _runner(_PlainElbmSim, model='bgk', entropic_equilibrium=True)[1].prepare()
    with pytest.raises(ValueError, match='BGK collision only'):
        _runner(_PlainElbmSim, model='elbm', regularized=True)[1].prepare()
    with pytest.raises(NotImplementedError, match='--incompressible'):
        _runner(_PlainElbmSim, model='elbm', incompressible=True, entropic_equilibrium=True)[1].prepare()


def test_alpha_travels_with_checkpoints(tmp_path):
    """The alpha field is state (the Newton start values of the next step): save_checkpoint stores the DEVICE copy,
    restore_checkpoint puts it back on the device."""
    cfg, r = _runner(_EntropicSim, tmp_path, max_iters=100)
    r.prepare()
    sim, b = r._sim, r.backend
    dev = r.gpu_field(sim.alpha)
    pattern = 1.5 + np.arange(sim.alpha.size, dtype=np.float64).reshape(sim.alpha.shape) / sim.alpha.size
    sim.alpha[...] = pattern
    b.to_buf(dev)
    sim.alpha[...] = -1.0                      # the host mirror is stale: the checkpoint must read the device
    sim.iteration = 4
    r.save_checkpoint()
    files = [f for f in os.listdir(str(tmp_path)) if f.endswith('.npz')]
    assert len(files) == 1
    saved = np.load(os.path.join(str(tmp_path), files[0]))
    assert 'field_alpha' in saved.files and np.array_equal(saved['field_alpha'], pattern)

    cfg2, r2 = _runner(_EntropicSim, tmp_path, max_iters=100)
    r2.prepare()
    assert np.all(r2._sim.alpha == 2.0)
    r2.restore_checkpoint(os.path.join(str(tmp_path), files[0]))
    assert r2._sim.iteration == 4
    assert np.array_equal(r2._sim.alpha, pattern)
    r2._sim.alpha[...] = 0.0
    r2.backend.from_buf(r2.gpu_field(r2._sim.alpha))
    assert np.array_equal(r2._sim.alpha, pattern)          # ... and it is on the device

    # a checkpoint of a simulation without the field restores into one with it (the start values stay 2)
    cfg3, r3 = _runner(_PlainElbmSim, tmp_path, model='elbm', checkpoint_file=os.path.join(str(tmp_path), 'plain'))
    r3.prepare()
    r3.save_checkpoint()
    plain = [f for f in os.listdir(str(tmp_path)) if f.startswith('plain')]
    assert 'field_alpha' not in np.load(os.path.join(str(tmp_path), plain[0])).files
    r2.restore_checkpoint(os.path.join(str(tmp_path), plain[0]))
    assert np.array_equal(r2._sim.alpha, pattern)
