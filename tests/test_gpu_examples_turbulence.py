"""examples/turbulence/channel_flow.py from the command line on the GPU, the way a user starts it, once for every wall
type (the pattern of tests/test_gpu_examples.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('wall', ['hbb', 'bbl', 'tms'])
def test_channel_flow_runs_from_the_command_line(wall, tmp_path):
    out = str(tmp_path / 'run')
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'turbulence', 'channel_flow.py'), '--H=8', '--Re_tau=20',
           '--max_iters=40', '--every=20', '--wall=' + wall, '--output=' + out, '--quiet',
           '--stats_after=0', '--stats_snapshots=1']      # statistics from the start, one snapshot per file
    res = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert res.returncode == 0, res.stdout.decode()[-2000:]
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith('run.') and f.endswith('.npz'))
    assert files, os.listdir(str(tmp_path))
    last = np.load(os.path.join(str(tmp_path), files[-1]))
    assert 'rho' in last.files and 'v' in last.files
    rho, v = last['rho'], last['v']
    assert rho.shape == (48, 16, 16 if wall == 'bbl' else 18)           # (6 H, 2 H, 2 H + the wall layers)
    assert np.isfinite(rho[~np.isnan(rho)]).all() and (~np.isnan(rho)).any()
    assert np.nanmax(v[2]) > 0.01                                       # the flow runs along z
    # the script's own sampling: a snapshot every 20 steps, each a file of profiles along x
    stats_dir = os.path.join(out, 'reyn_stats')
    stats = sorted(os.listdir(stats_dir))
    assert 'stats_0.40.npz' in stats, stats
    prof = np.load(os.path.join(stats_dir, 'stats_0.40.npz'))
    assert list(prof['iters']) == [40]
    assert 'uz_m1' in prof.files and np.max(prof['uz_m1']) > 0.01
    assert all(np.isfinite(prof[k]).all() for k in prof.files)
    assert all(prof[k].shape[-1] == rho.shape[-1] for k in prof.files if k != 'iters')
