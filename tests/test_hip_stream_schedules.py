"""The MB block backward under forced two-stream schedules.  `-m gpu`.

ofasr_mbconv_bwd runs the three weight gradients and the kernel-transform backward on the library's side stream beside
the input-gradient chain; with the deferred join (the default of ops.py) the side stream runs free until
flush_deferred().  What keeps that correct is hand-placed: the fork events, the liveness table of tA / tB / tC
(csrc/mbconv.hip, "who forms dy2 / dy1 on read") and the PendingSide waits for shared scratch.  The other GPU tests take
whatever schedule the GPU produces, and at their shapes the side kernels usually start long before the chain reaches
the buffer they read.  Here the schedule is an input (tests/stream_hold.py):

  natural  as the other tests run
  held     the side stream is held by one bounded spin until the whole input-gradient chain of the call has run
           (asserted from events: assert_held), so a chain kernel that overwrites what a side kernel still reads gives a
           wrong value on every run
  serial   OFASR_MBCONV_SIDE_STREAM=0 in ONE child process: every side kernel completes before the chain goes on

The path has no atomics and fixed summation orders, so dx, every parameter gradient and every region of the backward
scratch that holds a defined tensor at the end of the call are bit-identical under the three schedules; the held
schedule is also checked stage by stage against the CPU oracle (test_hip_composite16.check_block).

Sizing of the hold: each test first runs the same call unheld and times the caller's stream (events) and the host
across backward(); the hold is MARGIN = 4 x their sum, at least FLOOR_MS = 5 ms, at most MAX_HOLD_MS = 100 ms.
Measured on MI355X (the lines this module prints): torch.cuda._sleep spins 2.40e6 cycles per ms (two processes: 2398851,
2407805).  Chain / host time of backward() per block, second unheld run: 0.28 - 0.30 / 0.28 - 0.30 ms for the 64x64, 48x48
and 32x32 blocks with N <= 3, 0.38 / 0.38 ms at N = 5, 0.33 / 0.32 ms at 128x64 -- so every block hold is the 5 ms floor,
and the held chain was done 4.6 - 4.8 ms before the release.  (The first call of a block in a process took 800 ms to load
its kernels; hence the second run is the timed one.)  The whole-network passes of test_hip_deferred.py measured 1.6 - 2.3
ms of chain and as much host time per backward(): holds of 13 - 18 ms.
"""
import hashlib
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import stream_hold
import test_hip_composite16 as tb
from conftest import amd

pytestmark = pytest.mark.gpu
HERE = os.path.abspath(__file__)
BF16, F16 = torch.bfloat16, torch.float16

# (case, bstat): the smallest blocks that reach each side-stream kernel family and each row of the tA / tC table
BLOCKS = [
    ((2, 64, 64, 6, 7, True, BF16), False),    # dw_wgrad_mfma_kernel<..., true, true>: tA keeps da2, dy1 goes to tC
    ((2, 48, 48, 6, 3, True, BF16), False),    # vector weight gradient, one slab: dy2 in tC, dy1 over the dead da2 in tA
    ((3, 32, 32, 4, 5, True, BF16), False),    # second plane size
    ((2, 64, 64, 4, 5, True, F16), False),     # second 16-bit type
    ((2, 64, 64, 6, 7, False, BF16), False),   # eval-mode BN
    ((5, 64, 64, 6, 7, True, BF16), True),     # BN2 sums taken by the project input gradient (opt-in path)
    ((2, 128, 64, 3, 7, True, BF16), False),   # vector weight gradient, two slabs per plane (the K = 5 blocks: DESIGN.md 4)
]
BLOCK_ID = lambda b: ("bn2sums_in_dgrad-" if b[1] else "") + tb.CASE_ID(b[0])

# time limit of the child: 4 x the 3.4 s measured on the MI355X (start-up of the interpreter and the libraries, then the
# blocks), rounded up
CHILD_TIMEOUT = 20
FAULT_STATUS = (124, 134, 137, 139)
_NATURAL = {}    # block id -> {tensor name: sha256} of the natural schedule in this process
_STATE = {"dead": None}


def tensors_of(r, case):
    """what a schedule must not change: y, dx, every parameter gradient, the defined regions of the backward scratch"""
    N, Hh, Ww, e, K, train, dtype = case
    P, mid = N * Hh * Ww, r["mid"]
    bwd = r["bwd_table"]

    def ran(*parts):
        return sum(n for name, n in bwd.items() if all(p in name for p in parts))

    out = {"y": r["y"], "dx": r["dx"]}
    for n, g in r["grads"].items():
        out["grad:" + n] = g
    tmp = r["tmp"]
    out["tmp:tA"], out["tmp:tB"] = tmp[0:P * mid], tmp[P * mid:2 * P * mid]
    out["tmp:dy3"] = tmp[2 * P * mid:2 * P * mid + P * 64]
    # tC holds dy2 or dy1 where BN1 / BN2 backward are folded into their consumers, unless both weight gradients form
    # their operand on read (csrc/mbconv.hip)
    folded = ran("bn_bwd_apply_kernel") + ran("bn_bwd_onepass_kernel") == 1
    wg_bx = any("dw_wgrad_mfma_kernel" in k and k.rstrip().endswith("true, true>") for k in bwd)
    wg1 = ran("pw_wgrad_direct_kernel", ", 3>") > 0
    if folded and not (wg_bx and wg1):
        out["tmp:tC"] = tmp[2 * P * mid + P * 64:3 * P * mid + P * 64]
    return out


def sha(t):
    if t is None:
        return "None"
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def natural(block):
    """run_block under the natural schedule, twice (the first call of a kernel in a process also loads its code, so the
    second run is the one that is timed); the two runs must agree.  Remembers the hashes for the serial comparison"""
    case, bstat = block
    first = {k: sha(v) for k, v in tensors_of(tb.run_block(case, bstat), case).items()}
    timed = stream_hold.Timed()
    r = tb.run_block(case, bstat, timed)
    _NATURAL[BLOCK_ID(block)] = {k: sha(v) for k, v in tensors_of(r, case).items()}
    diff = [k for k in first if first[k] != _NATURAL[BLOCK_ID(block)][k]]
    assert not diff, "two runs under the natural schedule differ in %s" % diff
    return r, timed


@pytest.mark.parametrize("block", BLOCKS, ids=BLOCK_ID)
def test_block_held_equals_natural_and_oracle(ora, block):
    case, bstat = block
    r_nat, timed = natural(block)
    ms = timed.hold_ms()
    print("%s: chain %.3f ms, host %.3f ms -> hold %.1f ms at %.0f cycles/ms" % (
        BLOCK_ID(block), timed.chain_ms, timed.host_ms, ms, stream_hold.cycles_per_ms()))
    held = stream_hold.Held(ms)
    r_held = tb.run_block(case, bstat, held)
    print("  held run: the chain was done %.3f ms before the release" % held.check())
    t_nat, t_held = tensors_of(r_nat, case), tensors_of(r_held, case)
    assert list(t_nat) == list(t_held)
    diff = []
    for k in t_nat:
        assert (t_nat[k] is None) == (t_held[k] is None), "None-ness of %s" % k
        if t_nat[k] is not None and not torch.equal(t_nat[k], t_held[k]):
            d = (t_nat[k].float() - t_held[k].float()).abs()
            diff.append("%s: %d elements differ, max |diff| %g" % (k, int((d > 0).sum()), float(d.max())))
    assert not diff, "natural and held schedules differ:\n  " + "\n  ".join(diff)
    assert r_nat["bwd_table"] == r_held["bwd_table"]
    del r_nat, r_held, t_nat, t_held
    # the held schedule against the CPU oracle, stage by stage
    held2 = stream_hold.Held(ms)
    tb.check_block(ora, case, bstat, tb.DEFAULT_PROFILE, held2)
    held2.check()


def test_serial_schedule_equals_natural():
    """one child with the side stream off hashes the same tensors of every block"""
    if _STATE["dead"]:
        pytest.fail("not started: an earlier child faulted or hung (%s)" % _STATE["dead"])
    assert "OFASR_MBCONV_SIDE_STREAM" not in os.environ, "the parent must run with the side stream"
    for b in BLOCKS:
        if BLOCK_ID(b) not in _NATURAL:
            natural(b)
    torch.cuda.synchronize()
    env = dict(os.environ, OFASR_MBCONV_SIDE_STREAM="0")
    t0 = time.time()
    try:
        out = subprocess.run([sys.executable, HERE, "serial"], env=env, cwd=os.path.dirname(HERE), stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _STATE["dead"] = "the serial child ran into its %d s limit" % CHILD_TIMEOUT
        tail = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail("%s\n%s" % (_STATE["dead"], tail[-4000:]))
    print("serial child took %.1f s, status %d" % (time.time() - t0, out.returncode))
    if out.returncode < 0 or out.returncode in FAULT_STATUS:
        _STATE["dead"] = "the serial child ended with status %d" % out.returncode
    assert out.returncode == 0, "the serial child ended with status %d:\n%s" % (out.returncode, out.stdout[-4000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("HASHES ")]
    assert len(lines) == 1, out.stdout[-4000:]
    serial = json.loads(lines[0][7:])
    assert set(serial) == set(BLOCK_ID(b) for b in BLOCKS)
    diff = []
    for b in BLOCKS:
        mine, theirs = _NATURAL[BLOCK_ID(b)], serial[BLOCK_ID(b)]
        assert list(mine) == list(theirs), (BLOCK_ID(b), list(mine), list(theirs))
        diff += ["%s %s" % (BLOCK_ID(b), k) for k in mine if mine[k] != theirs[k]]
    assert not diff, "natural and serial schedules differ in:\n  " + "\n  ".join(diff)


def test_hold_refuses_long_holds():
    with pytest.raises(ValueError):
        stream_hold.hold(stream_hold.MAX_HOLD_MS + 1)


def _child_serial():
    assert os.environ.get("OFASR_MBCONV_SIDE_STREAM") == "0"
    assert amd("ops")._lib_side_stream(tb.DEV) is None, "the library ignored OFASR_MBCONV_SIDE_STREAM=0"
    try:
        stream_hold.hold(1.0)
    except RuntimeError:
        pass
    else:
        raise AssertionError("hold() must refuse when the side stream is disabled")
    hashes = {}
    for b in BLOCKS:
        case, bstat = b
        hashes[BLOCK_ID(b)] = {k: sha(v) for k, v in tensors_of(tb.run_block(case, bstat), case).items()}
    torch.cuda.synchronize()
    print("HASHES " + json.dumps(hashes))


if __name__ == "__main__":
    assert sys.argv[1:] == ["serial"], sys.argv
    _child_serial()
