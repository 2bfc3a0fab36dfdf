"""Which variants of the per-node sweep exist is stated once (csrc/slf_variant.h) and read by the launcher's instantiation
condition, by node_update's static_assert, by the launch bound and by module_config().  tests/variant_rule_main.cpp walks the
descriptors that select a variant and checks that statement against what module_config() accepts; it is built stand-alone,
with the address and undefined-behaviour sanitizers, and run directly."""
import os
import re
import shutil
import subprocess

import pytest

from tests import _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sailfish_amd', 'csrc')


@pytest.fixture(scope='module')
def rule_run(tmp_path_factory):
    done = _bind.run('variant_rule_main.cpp', tmp_path_factory.mktemp('variant_rule'), std='c++20')
    return done.returncode, [ln.split('\t') for ln in done.stdout.splitlines()], done.stderr


def test_accepted_modules_launch_existing_variants_within_their_bound(rule_run):
    """(a) and (b) of the program: every variant an accepted descriptor can launch exists and block_x respects its launch
    bound; the variants reached are exactly the ones instantiated."""
    code, lines, stderr = rule_run
    fails = [ln for ln in lines if ln[0] == 'fail']
    assert not fails, fails[:10]
    assert code == 0, stderr[-4000:]
    checked = [ln for ln in lines if ln[0] == 'checked'][0]
    # 2 lattices x 2 precisions x 3 models x 2 patterns x 2 x 2 x 3 density models x 2 x 2 x 2 x 2 x 2, at two row lengths
    assert int(checked[1]) == 2 * 2 * 3 * 2 * 2 * 2 * 3 * 2 * 2 * 2 * 2 * 2 * 2
    assert 0 < int(checked[2]) < int(checked[1])


def test_variant_count_matches_the_built_object(rule_run):
    """The number of distinct variants reached = the number of sweep_kernel instantiations in the built slf_kernels object
    (compared when a build is present)."""
    code, lines, _ = rule_run
    counts = {(int(ln[1]), int(ln[2])): int(ln[3]) for ln in lines if ln[0] == 'variants'}
    total = int([ln for ln in lines if ln[0] == 'total'][0][1])
    for key, n in sorted(counts.items()):
        print('lattice %d precision %d: %d variants' % (key + (n,)))
    assert set(counts) == {(0, 4), (0, 8), (1, 4), (1, 8)} and sum(counts.values()) == total and total > 0
    # the same rule in both precisions; shallow water adds its variants to D2Q9 only
    assert counts[0, 4] == counts[0, 8] and counts[1, 4] == counts[1, 8] and counts[0, 4] > counts[1, 4]
    obj = os.path.join(ROOT, 'sailfish_amd', 'lib', 'obj', 'slf_kernels.o')
    if os.path.exists(obj) and shutil.which('nm'):
        syms = subprocess.run(['nm', obj], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        kernels = set(re.findall(r'\b(_ZN3slf12sweep_kernelI\S+)', syms))
        assert len(kernels) == total
