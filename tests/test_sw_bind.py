"""The shallow-water model (slf_module_desc::equilibrium / gravity) in the library's HIP-free bind path (csrc/slf_bind.h):
which descriptors module_config() serves and how it configures them, what it refuses and with which words and code, that a
descriptor with both members zero gives what it gave before, and which kernel names such a module resolves.
tests/sw_bind_main.cpp is built stand-alone, with the address and undefined-behaviour sanitizers, and run directly."""
import os
import re

import pytest

from tests import _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sailfish_amd', 'csrc')
OK, INVALID, UNSUPPORTED, NOT_FOUND = 0, 1, 3, 4


@pytest.fixture(scope='module')
def bind_lines(tmp_path_factory):
    return _bind.lines('sw_bind_main.cpp', tmp_path_factory.mktemp('sw_bind'))


# subject -> (has_force, accel_field, block_x): a 4-node row is one wave; a 1000-node row one workgroup of 1024 threads, of
# 512 where the instantiation also reads the acceleration field (the ACCF launch bound)
SERVED = {'served': (0, 0, 64), 'served-aa-f64': (0, 0, 64), 'served-fluid-only': (0, 0, 64), 'served-wide': (0, 0, 1024),
          'served-wide-field': (1, 1, 512), 'served-force-edm': (1, 0, 64), 'served-field': (1, 1, 64)}
# subject -> the word the message must carry
REFUSED = {'d3q19': 'D2Q9 only', 'd3q15': 'D2Q9 only', 'mrt': '--model=mrt', 'elbm': '--model=elbm',
           'entropic_equilibrium': 'entropic_equilibrium', 'regularized': '--regularized', 'subgrid': '--subgrid',
           'minimize_roundoff': '--minimize_roundoff', 'incompressible': '--incompressible',
           'indirect': '--node_addressing=indirect', 'tms': 'NTWallTMS', 'equilibrium-density-node': 'carry a density or a velocity',
           'zouhe-velocity-node': 'carry a density or a velocity', 'regularized-velocity-node': 'carry a density or a velocity',
           'copy-node': 'carry a density or a velocity', 'do-nothing-node': 'carry a density or a velocity',
           'shan-chen-binary': 'Shan-Chen', 'shan-chen-single': 'Shan-Chen', 'free-energy': 'free-energy',
           'ternary': 'ternary Shan-Chen'}
INVALID_CASES = {'bad-equilibrium': 'equilibrium must be', 'negative-equilibrium': 'equilibrium must be',
                 'zero-gravity': 'gravity must be > 0', 'negative-gravity': 'gravity must be > 0'}
POLYNOMIAL = ('polynomial', 'polynomial-ignores-gravity', 'polynomial-wide')


def test_served_descriptors(bind_lines):
    rows = {ln[1]: ln for ln in bind_lines if ln[0] == 'config'}
    for subject, (force, field, bx) in SERVED.items():
        assert int(rows[subject][2]) == OK, rows[subject]
        # routed around the tuned, whole-row and slot kernels; the flag and the gravity reach the kernels' parameters
        assert rows[subject][4] == 'variant=0 equilibrium=1 gravity=0.05 has_force=%d accel_field=%d block_x=%d' % (force, field, bx), \
            rows[subject]


def test_zero_members_give_what_they_gave(bind_lines):
    """equilibrium = 0 (with or without a stray gravity): the polynomial's configuration -- no flag, no gravity, the default
    variant, whole rows of 1024 threads."""
    rows = {ln[1]: ln for ln in bind_lines if ln[0] == 'config'}
    for subject in POLYNOMIAL:
        assert int(rows[subject][2]) == OK, rows[subject]
        m = re.match(r'variant=(\d+) equilibrium=0 gravity=0 has_force=0 accel_field=0 block_x=(\d+)$', rows[subject][4])
        assert m and int(m.group(1)) != 0, rows[subject]
        assert int(m.group(2)) == (1024 if subject == 'polynomial-wide' else 64)
    assert rows['polynomial'][4] == rows['polynomial-ignores-gravity'][4]


def test_refusals_name_the_option(bind_lines):
    rows = {ln[1]: ln for ln in bind_lines if ln[0] == 'config'}
    assert set(REFUSED) | set(SERVED) | set(INVALID_CASES) | set(POLYNOMIAL) == set(rows)
    for subject, word in REFUSED.items():
        code, msg = int(rows[subject][2]), rows[subject][3]
        assert code == UNSUPPORTED and msg.startswith('shallow water: ') and word in msg, rows[subject]
    for subject, word in INVALID_CASES.items():
        code, msg = int(rows[subject][2]), rows[subject][3]
        assert code == INVALID and word in msg, rows[subject]


def test_kernel_names_of_a_shallow_water_module(bind_lines):
    """No new names: such a module answers to the names of any single-fluid module, with the same kernel kinds; the
    several-steps-per-launch kernel alone does not exist in it."""
    rows = {ln[1]: ln for ln in bind_lines if ln[0] == 'resolve'}
    table = set(re.findall(r'^  \{"(\w+)", KK_', open(os.path.join(CSRC, 'slf_bind.h')).read(), re.M))
    assert len(table) >= 25
    assert set(rows) == set(n + s for n in table for s in ('-sw', '-plain'))
    for name in table:
        sw, plain = rows[name + '-sw'], rows[name + '-plain']
        if name == 'CollideAndPropagateResident':
            assert int(plain[2]) == OK
            assert int(sw[2]) == UNSUPPORTED and 'shallow-water' in sw[3] and 'CollideAndPropagateResident' in sw[3]
        else:
            assert sw[2:] == plain[2:], name          # same code, message and kernel kind
    for name in ('CollideAndPropagate', 'SetInitialConditions', 'ComputeMacroFields', 'ApplyPeriodicBoundaryConditions'):
        assert int(rows[name + '-sw'][2]) == OK


def test_header_binding_and_predicate_in_step():
    """equilibrium and gravity sit at the same place in the header's slf_module_desc and in hipabi.SlfModuleDesc: in what were
    the two padding holes in front of tau and of node_params.  No other member moves and the structure keeps its 760 bytes
    (tests/test_accf_bind.py pins them), which is why gravity is a float; the three entropic members stay last and the ABI
    version stays 1."""
    from sailfish_amd import hipabi
    src = open(os.path.join(ROOT, 'include', 'sailfish_hip.h')).read()
    body = src[src.index('typedef struct slf_module_desc {'):src.index('} slf_module_desc;')]
    assert body.index('int32_t fluid_only;') < body.index('int32_t equilibrium;') < body.index('double tau;')
    assert body.index('int32_t n_node_params;') < body.index('float gravity;') < body.index('const double* node_params;')
    names = [f[0] for f in hipabi.SlfModuleDesc._fields_]
    i, j = names.index('equilibrium'), names.index('gravity')
    assert names[i - 1:i + 2] == ['fluid_only', 'equilibrium', 'tau'] and names[j - 1:j + 2] == ['n_node_params', 'gravity', 'node_params']
    assert names[-3:] == ['entropic_equilibrium', 'entropy_tolerance', 'alpha_tolerance']
    D = hipabi.SlfModuleDesc
    assert hipabi.ctypes.sizeof(D) == 760
    assert (D.fluid_only.offset, D.equilibrium.offset, D.tau.offset) == (72, 76, 80)
    assert (D.n_node_params.offset, D.gravity.offset, D.node_params.offset) == (424, 428, 432)
    assert (D.accel_field.offset, D.alpha_tolerance.offset) == (624, 752) and D.gravity.size == 4
    assert re.search(r'#define SLF_ABI_VERSION 1\b', src)
    assert re.search(r'enum \{ SLF_EQ_BGK = 0, SLF_EQ_SHALLOW_WATER = 1 \};', src)
    assert (hipabi.SLF_EQ_BGK, hipabi.SLF_EQ_SHALLOW_WATER) == (0, 1)
    plain = hipabi.make_desc()
    assert plain.equilibrium == 0 and plain.gravity == 0.0 and plain.struct_size == 760
    bind = open(os.path.join(CSRC, 'slf_bind.h')).read()
    # the rows that serve the feature are in the support table, in front of module_config() which walks it
    assert bind.index('{"shallow water", SLF_HAS(') < bind.index('{"accel_field", SLF_HAS(') < bind.index('SLF_LAT_ROW("D3Q15", ') < \
        bind.index('inline const char* serves_conflict') < bind.index('inline int module_config')
