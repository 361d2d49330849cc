"""A bounded hold of the library's side stream, so that a test can choose which stream gets ahead.

The weight-gradient kernels of the MB block backward wait for fork events on the library's side stream
(ops._lib_side_stream, csrc/mbconv.hip); the input-gradient chain on the caller's stream waits for nothing until the
join.  One bounded spin (torch.cuda._sleep) put on the side stream before backward() therefore lets the whole chain of
the call run before any side kernel starts: every "the chain overwrites what a side kernel still reads" hazard then
gives a wrong value on every run instead of now and then.  OFASR_MBCONV_SIDE_STREAM=0 is the opposite extreme (every
side kernel completes before the chain goes on); a correct library gives the same bits under all schedules.

Only a device-side delay with a fixed cycle count is used: nothing waits for the host, nothing spins on a flag, and no
single hold is longer than MAX_HOLD_MS.  A hold that turned out too short is caught by assert_held, never passed over."""
import time

import torch

from conftest import amd

MAX_HOLD_MS = 100.0     # upper limit of one hold
FLOOR_MS = 5.0          # lower limit of a sized hold: covers the calibration error (a few per cent) and event jitter
MARGIN = 4.0            # hold = MARGIN x (chain time + host time to enqueue); assert_held guards against under-sizing
_PROBE_MS = 4.0         # length of the calibration spin
_CAL = {}               # device index -> spin cycles per millisecond


def side_stream(dev="cuda:0"):
    side = amd("ops")._lib_side_stream(dev)
    if side is None:
        raise RuntimeError("the library's side stream is disabled (OFASR_MBCONV_SIDE_STREAM=0): nothing to hold")
    return side


def cycles_per_ms(dev="cuda:0"):
    """spin cycles of torch.cuda._sleep per millisecond on `dev`, measured once per process with events"""
    key = torch.device(dev).index or 0
    if key not in _CAL:
        side = side_stream(dev)
        torch.cuda.synchronize()

        def timed(cycles):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record(side)
                torch.cuda._sleep(int(cycles))
                e1.record(side)
            e1.synchronize()
            return e0.elapsed_time(e1)

        timed(10000)                                   # first launch of the spin kernel
        rough = 200000 / max(timed(200000), 1e-3)      # cycles per ms, from a spin of at most a few ms
        probe = int(min(rough * _PROBE_MS, 2e9))
        _CAL[key] = probe / max(timed(probe), 1e-3)
        print("stream_hold: %.0f spin cycles per ms (probe of %d cycles)" % (_CAL[key], probe))
    return _CAL[key]


def hold_ms_for(chain_ms, host_ms):
    """size of the hold for a call whose chain took `chain_ms` on the caller's stream and `host_ms` to enqueue"""
    return min(MAX_HOLD_MS, max(FLOOR_MS, MARGIN * (chain_ms + host_ms)))


def hold(ms, dev="cuda:0"):
    """keep the side stream busy for `ms` milliseconds from now on (one bounded spin); returns the event recorded on the
    side stream behind the spin"""
    if not 0 < ms <= MAX_HOLD_MS:
        raise ValueError("a hold is at most %g ms, not %g" % (MAX_HOLD_MS, ms))
    side = side_stream(dev)
    cycles = int(ms * cycles_per_ms(dev))
    released = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        released.record(side)
    return released


def assert_held(released, main_done):
    """the caller's stream had reached `main_done` before the side stream was released"""
    torch.cuda.synchronize()
    lead = main_done.elapsed_time(released)
    assert lead >= 0, "the hold ended %.3f ms before the input-gradient chain did: this was not the held schedule" % -lead
    return lead


class Timed(object):
    """before_backward hook of the unheld run: times the caller's stream and the host across backward()"""

    def __init__(self):
        self.chain_ms = self.host_ms = None

    def __call__(self, stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()

        def after(stream_):
            self.host_ms = (time.perf_counter() - t0) * 1e3
            e1.record(stream_)
            e1.synchronize()
            self.chain_ms = e0.elapsed_time(e1)
        return after

    def hold_ms(self):
        return hold_ms_for(self.chain_ms, self.host_ms)


class Held(object):
    """before_backward hook of the held run: holds the side stream for `ms`, records main_done behind backward()"""

    def __init__(self, ms, dev="cuda:0"):
        self.ms, self.dev, self.released, self.main_done = ms, dev, None, None

    def __call__(self, stream):
        cycles_per_ms(self.dev)        # calibrate before the hold starts, not inside it
        self.released = hold(self.ms, self.dev)

        def after(stream_):
            self.main_done = torch.cuda.Event(enable_timing=True)
            self.main_done.record(stream_)
        return after

    def check(self):
        return assert_held(self.released, self.main_done)
