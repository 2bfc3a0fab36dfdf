"""The argument checks of the thermal entry points (slf_thermal_*; csrc/slf_bind.h thermal_check), HIP-free.
tests/thermal_bind_main.cpp is built stand-alone, with the address and undefined-behaviour sanitizers, and run directly as a
child process: nothing is loaded into Python."""
import ctypes
import os
import re

import pytest

from sailfish_amd import hipabi
from tests import _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sailfish_amd', 'csrc')
OK, INVALID, UNSUPPORTED = 0, 1, 3


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    done = _bind.run('thermal_bind_main.cpp', tmp_path_factory.mktemp('thermal_bind'))
    assert done.returncode == 0, done.stderr[-4000:]
    return {ln.split('\t')[0]: ln.split('\t') for ln in done.stdout.splitlines()}


SERVED = ('served-d2q9', 'served-d3q19-f64', 'served-with-map')
REFUSED = {'no-accel-field': (INVALID, 'accel_field'), 'field-not-set': (INVALID, 'slf_module_set_accel_field'),
           'null-params': (INVALID, 'params is NULL'), 'omega-zero': (INVALID, 'omega_T'), 'omega-two': (INVALID, 'omega_T'),
           'omega-negative': (INVALID, 'omega_T'), 'omega-nan': (INVALID, 'omega_T'),
           'buoyancy-not-finite': (INVALID, 'finite'), 't-ref-nan': (INVALID, 'finite'),
           'null-map-with-node-types': (INVALID, 'map is NULL'), 'null-g-src': (INVALID, 'g_src is NULL'),
           'null-t': (INVALID, 'T is NULL'), 'src-is-dst': (INVALID, 'g_src == g_dst'),
           'd3q15': (UNSUPPORTED, 'D3Q15'), 'd3q27': (UNSUPPORTED, 'D3Q15 / D3Q27')}


def test_bind_program_walks_the_argument_checks(rows):
    assert set(SERVED) | set(REFUSED) == set(rows)
    for subject in SERVED:
        assert int(rows[subject][1]) == OK, rows[subject]
    for subject, (code, word) in REFUSED.items():
        assert int(rows[subject][1]) == code and word in rows[subject][2], rows[subject]
        assert rows[subject][2].startswith('slf_thermal_test: ')


def test_header_and_binding():
    """The two entry points are declared and bound, the parameter structure has the C layout, the ABI version stays 1, and
    neither slf_module_desc nor the kernel table knows about the temperature lattice."""
    src = open(os.path.join(ROOT, 'include', 'sailfish_hip.h')).read()
    assert re.search(r'#define SLF_ABI_VERSION 1\b', src)
    assert 'int slf_thermal_init(slf_module* m, const slf_thermal_params* params' in src
    assert 'int slf_thermal_step(slf_module* m, const slf_thermal_params* params' in src
    assert len(hipabi.SIGNATURES['slf_thermal_init'][1]) == 9 and len(hipabi.SIGNATURES['slf_thermal_step'][1]) == 11
    P = hipabi.SlfThermalParams
    assert ctypes.sizeof(P) == 56 and (P.omega_T.offset, P.T_ref.offset, P.b.offset, P.periodic.offset, P.reserved.offset) == \
        (0, 8, 16, 40, 52)
    body = src[src.index('typedef struct slf_thermal_params {'):src.index('} slf_thermal_params;')]
    order = [body.index(w) for w in ('double omega_T;', 'double T_ref;', 'double b[3];', 'int32_t periodic[3];', 'int32_t reserved;')]
    assert order == sorted(order)
    desc = src[src.index('typedef struct slf_module_desc {'):src.index('} slf_module_desc;')]
    assert 'thermal' not in desc.lower()
    bind = open(os.path.join(CSRC, 'slf_bind.h')).read()
    table = bind[bind.index('KERNEL_TABLE[] = {'):]
    assert 'hermal' not in table[:table.index('\n};')]
