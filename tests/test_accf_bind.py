"""The acceleration field (slf_module_desc::accel_field) in the library's HIP-free bind path (csrc/slf_bind.h): which
descriptors module_config() serves, what it refuses and with which words, and which kernel names such a module resolves.
tests/accf_bind_main.cpp is built stand-alone, with the address and undefined-behaviour sanitizers, and run directly."""
import os
import re

import pytest

from tests import _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sailfish_amd', 'csrc')
OK, INVALID, UNSUPPORTED, NOT_FOUND = 0, 1, 3, 4


@pytest.fixture(scope='module')
def bind_lines(tmp_path_factory):
    return _bind.lines('accf_bind_main.cpp', tmp_path_factory.mktemp('accf_bind'))


SERVED = ('served-d2q9', 'served-d3q19', 'served-d3q19-mrt-aa-f64', 'served-d2q9-edm-incompressible-uniform-part',
          'served-d3q19-fluid-only', 'served-d3q19-boundary-conditions')
# subject -> the word the message must carry
REFUSED = {'d3q15': 'D3Q15', 'd3q27': 'D3Q27', 'elbm': '--model=elbm', 'regularized': '--regularized', 'subgrid': '--subgrid',
           'minimize_roundoff': '--minimize_roundoff', 'tms': 'NTWallTMS', 'indirect': '--node_addressing=indirect',
           'shan-chen-binary': 'Shan-Chen', 'shan-chen-single': 'Shan-Chen', 'free-energy': 'free-energy',
           'ternary': 'ternary Shan-Chen'}


def test_served_descriptors(bind_lines):
    rows = {ln[1]: ln for ln in bind_lines if ln[0] == 'config'}
    for subject in SERVED:
        assert int(rows[subject][2]) == OK, rows[subject]
        # routed around the tuned, whole-row and slot kernels; a field is a body force
        assert rows[subject][4] == 'variant=0 has_force=1 accel_field=1', rows[subject]
    plain = rows['no-field-d3q19']
    assert int(plain[2]) == OK and plain[4].endswith('has_force=0 accel_field=0') and plain[4] != 'variant=0 has_force=0 accel_field=0'


def test_refusals_name_the_option(bind_lines):
    rows = {ln[1]: ln for ln in bind_lines if ln[0] == 'config'}
    assert set(REFUSED) | set(SERVED) | {'no-field-d3q19', 'bad-flag', 'mrt-edm'} == set(rows)
    for subject, word in REFUSED.items():
        code, msg = int(rows[subject][2]), rows[subject][3]
        assert code == UNSUPPORTED and msg.startswith('accel_field: ') and word in msg, rows[subject]
    assert int(rows['bad-flag'][2]) == INVALID and 'accel_field must be 0 or 1' in rows['bad-flag'][3]
    # the exact difference method stays BGK only, with or without a field
    assert int(rows['mrt-edm'][2]) == UNSUPPORTED and 'exact difference method' in rows['mrt-edm'][3]


def test_kernel_names_of_a_module_with_a_field(bind_lines):
    rows = {ln[1]: ln for ln in bind_lines if ln[0] == 'resolve'}
    table = set(re.findall(r'^  \{"(\w+)", KK_', open(os.path.join(CSRC, 'slf_bind.h')).read(), re.M))
    assert len(table) >= 25
    assert set(rows) == set(n + s for n in table for s in ('-field', '-plain'))
    for name in table:
        field, plain = rows[name + '-field'], rows[name + '-plain']
        if name == 'CollideAndPropagateResident':
            assert int(plain[2]) == OK
            assert int(field[2]) == UNSUPPORTED and 'accel_field' in field[3] and 'CollideAndPropagateResident' in field[3]
        else:
            assert field[2:] == plain[2:], name          # same code, message and kernel kind


def test_header_binding_and_predicate_in_step():
    """accel_field sits at the same place in the header's slf_module_desc and in hipabi.SlfModuleDesc -- between the
    free-energy and the ternary members, where it lengthens the structure (a caller built against the earlier layout fails
    the struct_size check) --, the ABI version stays 1 and the entry point is declared and bound."""
    from sailfish_amd import hipabi
    src = open(os.path.join(ROOT, 'include', 'sailfish_hip.h')).read()
    body = src[src.index('typedef struct slf_module_desc {'):src.index('} slf_module_desc;')]
    assert body.index('int32_t fe_zero_grad_rim[3];') < body.index('int32_t accel_field;') < body.index('double tau_theta;')
    names = [f[0] for f in hipabi.SlfModuleDesc._fields_]
    assert names[names.index('accel_field') - 1] == 'fe_zero_grad_rim' and names[names.index('accel_field') + 1] == 'tau_theta'
    assert hipabi.ctypes.sizeof(hipabi.SlfModuleDesc) == 760 and hipabi.SlfModuleDesc.accel_field.offset == 624
    assert re.search(r'#define SLF_ABI_VERSION 1\b', src)
    assert 'int slf_module_set_accel_field(slf_module* m, void* field);' in src
    assert 'slf_module_set_accel_field' in hipabi.SIGNATURES
    bind = open(os.path.join(CSRC, 'slf_bind.h')).read()
    # the rows that serve the feature are in the support table, in front of module_config() which walks it
    assert bind.index('{"shallow water", SLF_HAS(') < bind.index('{"accel_field", SLF_HAS(') < bind.index('SLF_LAT_ROW("D3Q15", ') < \
        bind.index('inline const char* serves_conflict') < bind.index('inline int module_config')
