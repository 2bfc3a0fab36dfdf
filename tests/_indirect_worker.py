"""Worker of tests/test_gpu_indirect.py: runs cases of tests/_indirect_sims.py through the controller in a process of its
own and writes the merged fields.  The library reads SLF_INDIRECT_SLOTS once per process, so the per-node indirect sweep
(SLF_INDIRECT_SLOTS=0) can only be reached from a fresh process.
usage: _indirect_worker.py <output directory> <case name> [<case name> ...]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np

from tests import _indirect_sims as S
from tests.test_gpu_runner import merged_gpu, run_gpu


def fields_of(ctrl, dim):
    out = {'rho': merged_gpu(ctrl, 'rho'), 'dist': merged_gpu(ctrl, 'dist')}
    out['v'] = np.stack([merged_gpu(ctrl, 'v%d' % d) for d in range(dim)])
    return out


def run_case(name):
    case = S.CASES[name]
    ctrl = run_gpu(S.sim_class(case), None, case['dim'], case['cfg'], case['steps'])
    assert all(r._desc.node_addressing == 1 for r in ctrl.runners)
    res = fields_of(ctrl, case['dim'])
    for r in ctrl.runners:
        r.release()
    return res


if __name__ == '__main__':
    out_dir, names = sys.argv[1], sys.argv[2:]
    print('SLF_INDIRECT_SLOTS=%s' % os.environ.get('SLF_INDIRECT_SLOTS'), flush=True)
    for name in names:
        for what, arr in run_case(name).items():
            np.save(os.path.join(out_dir, '%s.%s.npy' % (name, what)), arr)
        print('done', name, flush=True)
