"""Deferred pair stepping of the box driver (sailfish_amd/box.py) as pure host code: a backend that only records which
kernel object is launched (the style of tests/_recording_queue.py) -- which launch every sequence of calls produces,
and that `gpu_dist[iteration & 1]` names the array that holds the state of `iteration` after each of them."""
import numpy as np
import pytest

from sailfish_amd import sym
from sailfish_amd.box import BoxSim, make_box_desc


class Stream(object):
    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append(('sync',))


class Kernel(object):
    def __init__(self, name, args):
        self.name, self.args, self.pair = name, list(args), False
        self.needs_iteration = False


class Module(object):
    block_size = 64


class RecordingBackend(object):
    """Hands out addresses and kernel objects, performs nothing, logs launches and copies.  `where` follows the data:
    the array address that holds the state of which step."""

    def __init__(self, accept=True):
        self.log, self.accept, self.next_addr = [], accept, 0x1000
        self.state = {}         # array address -> step whose populations it holds

    def build(self, desc):
        return Module()

    def dist_align_offset(self, itemsize):
        return 0

    def alloc_buf(self, size=None, like=None, align_offset=0):
        self.next_addr += 0x1000
        return self.next_addr

    def free_buf(self, addr):
        pass

    def make_stream(self):
        return Stream(self.log)

    def supports_row_classes(self, desc):
        return False

    def get_kernel(self, module, name, block, args, fmt, needs_iteration=False):
        return Kernel(name, args)

    def set_kernel_pair(self, kernel, rows=0, zchunk=0):
        if not self.accept:
            return 'refused by the test'
        kernel.pair = True
        return None

    def set_iteration(self, it):
        pass

    def to_buf(self, buf, source=None):
        pass

    def from_buf(self, buf, target=None):
        self.log.append(('read', buf))

    def run_kernel(self, kernel, region=None, stream=None):
        if kernel.name == 'SetInitialConditions':
            self.state[kernel.args[0]] = 0
            return
        assert kernel.name == 'CollideAndPropagate'
        src, dst = kernel.args[1], kernel.args[2]
        steps = 2 if kernel.pair else 1
        self.state[dst] = self.state[src] + steps
        self.log.append(('pair' if kernel.pair else ('single+macro' if kernel.args[-1] else 'single'), src, dst))

    def copy_dist_async(self, dst, src, nbytes, stream=None):
        self.state[dst] = self.state[src]
        self.log.append(('copy', src, dst))


def make(accept=True, monkeypatch=None):
    b = RecordingBackend(accept)
    desc = make_box_desc(sym.D3Q19, (64, 4, 4), precision='single', access_pattern='AB', visc=0.02,
                         periodic_fused=[1, 1, 1])
    s = BoxSim(b, desc, periodic=(True, True, True))
    s.initial_conditions()
    return b, s


def launches(b):
    return [e[0] for e in b.log if e[0] in ('pair', 'single', 'single+macro', 'copy')]


def current_is_right(b, s):
    """After a flush the array gpu_dist[iteration & 1] holds step `iteration`."""
    assert b.state[s.gpu_dist[s.iteration & 1]] == s.iteration


def test_first_step_is_deferred_and_second_launches_the_pair():
    b, s = make()
    a0 = list(s.gpu_dist)
    s.step()
    assert launches(b) == [] and s.iteration == 1
    s.step()
    assert launches(b) == ['pair'] and s.iteration == 2
    # the pair read copy 0 and wrote copy 1; the parity of the iteration is what it was: the list turned round, in place
    assert b.log[-1] == ('pair', a0[0], a0[1])
    assert s.gpu_dist == [a0[1], a0[0]]
    assert b.state[s.gpu_dist[s.iteration & 1]] == 2


@pytest.mark.parametrize('n', [1, 2, 3, 7, 8])
def test_n_steps_then_sync(n):
    b, s = make()
    a0 = list(s.gpu_dist)
    for _ in range(n):
        s.step()
    s.sync()
    want = ['pair'] * (n // 2) + (['single'] if n & 1 else [])
    # an odd number of pair launches leaves the populations in the array single steps would not: copied over at the flush
    want += ['copy'] if (n // 2) & 1 else []
    assert launches(b) == want
    assert s.iteration == n and s.gpu_dist == a0
    current_is_right(b, s)
    assert s.pair_launches == n // 2


def test_sync_between_steps_flushes_with_the_single_step_kernel():
    b, s = make()
    s.step()
    s.sync()
    assert launches(b) == ['single']
    current_is_right(b, s)
    s.step()
    s.step()
    s.get_dist()
    assert launches(b) == ['single', 'pair', 'copy']
    current_is_right(b, s)
    assert b.log[-1] == ('read', s.gpu_dist[s.iteration & 1])


def test_step_with_fields_flushes_first():
    b, s = make()
    s.step()
    s.step(save_macro=True)
    assert launches(b) == ['single', 'single+macro'] and s.iteration == 2
    s.sync()
    current_is_right(b, s)
    # ... and after a pair launch the single-step kernels come from the lists that turned round with the arrays
    s.step()
    s.step()
    s.step()
    s.step(save_macro=True)
    assert launches(b)[2:] == ['pair', 'single', 'single+macro']
    s.sync()
    assert s.iteration == 6
    current_is_right(b, s)


def test_region_steps_never_pair():
    b, s = make()
    for _ in range(2):
        s.step(region=(1, 5, 1, 3))
    assert launches(b) == ['single', 'single']


def test_set_dist_and_initial_conditions_flush():
    b, s = make()
    s.step()
    s.set_dist(np.zeros((19,) + s.shape, dtype=np.float32))
    assert launches(b) == ['single']
    for _ in range(3):
        s.step()
    s.initial_conditions()
    assert launches(b) == ['single', 'pair', 'single', 'copy'] and s.iteration == 0
    s.step()
    s.step()
    s.sync()
    assert launches(b)[4:] == ['pair', 'copy']
    current_is_right(b, s)


def test_a_refusal_means_single_steps(monkeypatch):
    b, s = make(accept=False)
    assert s.k_pair is None and s.pair_refused == 'refused by the test'
    for _ in range(4):
        s.step()
    s.sync()
    assert launches(b) == ['single'] * 4
    current_is_right(b, s)


def test_switch(monkeypatch):
    monkeypatch.setenv('SLF_STEP_PAIRS', '0')
    b, s = make()
    assert s.k_pair is None
    s.step()
    assert launches(b) == ['single']
