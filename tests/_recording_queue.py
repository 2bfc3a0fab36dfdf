"""A step queue (the interface of sailfish_amd/stepqueue.DirectQueue) that performs nothing and logs every entry as
(op, stream, event / kernel, region) -- for tests of the step programs as pure host code.  Streams and events are
stand-in objects: only their identity counts."""


class Stub(object):
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


class RecordingQueue(object):
    planned = False

    def __init__(self):
        self.log = []

    def launch(self, kernel, region, stream):
        self.log.append(('launch', stream, kernel, region))

    def record(self, event, stream):
        self.log.append(('record', stream, event, None))

    def wait(self, stream, event):
        self.log.append(('wait', stream, event, None))

    def exchange(self, rccl, batch, stream):
        self.log.append(('exchange', stream, batch, None))

    def peer_signal(self, peer, ranks, channel, stream):
        self.log.append(('peer_signal', stream, channel, None))

    def peer_wait(self, peer, ranks, channel, stream, count=1):
        self.log.append(('peer_wait', stream, channel, count))

    def memset(self, addr, value, nbytes, stream):
        self.log.append(('memset', stream, addr, nbytes))

    def copy(self, dst, src, nbytes, stream):
        self.log.append(('copy', stream, (dst, src), nbytes))

    def xface(self, module, send_low, send_high, recv_low, recv_high):
        self.log.append(('xface', None, module, (send_low, send_high, recv_low, recv_high)))

    def xface_planes(self, module, which, send_low, send_high, recv_low, recv_high):
        self.log.append(('xface_planes', None, module, (which, send_low, send_high, recv_low, recv_high)))

    def call(self, fn):
        self.log.append(('call', None, fn, None))
