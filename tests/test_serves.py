"""The support table exists twice: SERVES in sailfish_amd/csrc/slf_bind.h, which the library walks at module creation, and
ROWS in sailfish_amd/serves.py, which the host walks before anything is built.  tests/abi_bind_main.cpp prints the C table in
its `serves` section, one line per row; tests/test_abi_bind.py holds that output equal to tests/golden/abi_support.tsv, and
this test holds the recorded lines equal to the Python rows: names, order, per_node_only and every mask."""
import os
import re

from sailfish_amd import serves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_python_rows_are_the_c_rows():
    c_rows = []
    for ln in open(os.path.join(ROOT, 'tests', 'golden', 'abi_support.tsv')).read().splitlines():
        section, name, _, position, per_node_only, _, masks = ln.split('\t') if ln.startswith('serves\t') else [None] * 7
        if section:
            assert position == 'row%d' % len(c_rows)
            c_rows.append((name, int(per_node_only), tuple(int(m) for m in masks.split())))
    src = open(os.path.join(ROOT, 'sailfish_amd', 'csrc', 'slf_bind.h')).read()
    assert len(c_rows) == len(serves.ROWS) >= 11
    py_rows = [(r.name, int(r.per_node_only), tuple(r.serves)) for r in serves.ROWS]
    for c, py in zip(c_rows, py_rows):
        assert c == py, (c, py)
    assert all(len(r.serves) == len(serves.COLUMNS) for r in serves.ROWS)
    # the columns are the header's, in its order
    columns = re.search(r'enum Column \{([^}]*)\}', src).group(1)
    assert [c.strip() for c in columns.split(',')][:-1] == ['COL_LATTICE', 'COL_SIMTYPE', 'COL_MODEL', 'COL_ENTROPIC', 'COL_REGULARIZED',
                                                             'COL_SUBGRID', 'COL_DENSITY', 'COL_ADDRESSING', 'COL_FORCE', 'COL_ACCEL_FIELD',
                                                             'COL_EDM', 'COL_KINDS']
    words = src[src.index('} COLUMNS[N_COLUMNS] = {'):src.index('// A row is a feature')]
    assert re.findall(r'^  \{(?:&slf_module_desc::\w+|nullptr), "(\w+)", \d+,', words, re.M) == list(serves.COLUMNS)
