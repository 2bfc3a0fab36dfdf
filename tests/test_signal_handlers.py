"""SIGHUP -> checkpoint request (SubdomainRunner._install_signal_handlers) in a process that runs many simulations one
after the other, as the test suite does: one handler for the process, every live runner gets the request, runners that
are gone are forgotten.  (A handler per runner that called the one before it ended in a RecursionError once a process
had prepared about a thousand runners: tests/test_gpu_runner.py::test_sighup_triggers_checkpoint late in the suite.)"""
import gc
import os
import signal

from sailfish_amd import subdomain_runner as sr


class _Stub(sr.SubdomainRunner):
    def __init__(self):
        self.got = 0

    def sighup_handler(self, signum, frame):
        self.got += 1


def test_sighup_reaches_every_live_runner_through_one_handler():
    old = signal.getsignal(signal.SIGHUP)
    seen = []
    try:
        signal.signal(signal.SIGHUP, lambda signum, frame: seen.append(signum))     # what the host program had installed
        keep = []
        for i in range(3000):
            r = _Stub()
            r._install_signal_handlers()
            if i % 1000 == 0:
                keep.append(r)
        del r
        gc.collect()
        assert signal.getsignal(signal.SIGHUP) is sr._hup_dispatch
        os.kill(os.getpid(), signal.SIGHUP)
        assert [r.got for r in keep] == [1, 1, 1]
        assert seen == [signal.SIGHUP]                      # the earlier handler is still served, once
        assert all(r in sr._hup_runners for r in keep)
        assert sum(isinstance(r, _Stub) for r in list(sr._hup_runners)) == len(keep)
        # the host program takes the signal back: the next runner installs the dispatcher again, once
        signal.signal(signal.SIGHUP, old)
        late = _Stub()
        late._install_signal_handlers()
        late._install_signal_handlers()
        if callable(old) or old in (signal.SIG_IGN,):
            os.kill(os.getpid(), signal.SIGHUP)
            assert late.got == 1 and [r.got for r in keep] == [2, 2, 2]
    finally:
        signal.signal(signal.SIGHUP, old)
