"""The streaming operand path of the 16-bit pointwise weight gradient (pw_wgrad_direct_kernel, csrc/pw_wgrad_stream.h):
both operands reach LDS as whole 128-byte lines by LDS-DMA, a fragment is one LDS read.

Every case runs through the C ABI on guard-banded operands (tests/placed.py: NaN directly before the first and after
the last element of every input, so a read outside a tensor poisons the result -- placed.py puts no tensor at the end
of an allocation, the NaN band is its stand-in for that; canaries around the output and the workspace, which has
exactly the queried size), with the plain read and with
the fused BN + ReLU6 input transform, and is compared with the CPU oracle at the bar of
test_hip_kernels.py::test_pwconv_vs_oracle for the weight gradient: rtol 1e-4, atol 2e-6 * sqrt(N * HW).

The transform's constants are dyadic (scale 2 / 4 / 8, mean and shift multiples of 1/4), so v -> (v - mean) * scale +
shift + mean * scale is exact in fp32 for 16-bit v and the only rounding is the final one to the 16-bit type, which the
reference makes the same way; with v in [-1, 1] the results spread over [-7.5, 13.5]: below 0, inside (0, 6), above 6.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd, assert_close
from detfill import det_uniform
from placed import check, place, workspace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F16 = torch.bfloat16, torch.float16
CODE = {torch.float32: 0, F16: 1, BF16: 2}   # fp32: the rows of tests/test_hip_switches.py that call run() on fp32 operands
TNAME = {F16: "ofasr::f16_t", BF16: "ofasr::bf16_t"}

SHAPES = [
    # (N, narrow, wide, HW)
    (1, 64, 384, 64),      # one stage
    (1, 64, 384, 192),     # exactly one ring turn
    (2, 64, 192, 1024),    # row tile partly empty: one 192-row tile, no second
    (2, 64, 256, 2304),    # 48 x 48, ragged second row tile (64 of 192 rows)
    (3, 64, 384, 4096),    # many turns
    (1, 60, 380, 128),     # NS < 64, MR % 32 != 0
    (1, 64, 384, 832),     # 13 stages over 3 splits: the stage count is not divisible by the splits
    (8, 64, 200, 2048),    # 256 stages = 64 splits: a whole group of the reduce launch, so splits z and z + 16 share a slab
]
ROLES = ["expand", "project"]   # expand: Cout (wide) >= Cin, x is the narrow operand; project: Cin (wide) > Cout


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return amd("_C").lib()


def rounded(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def G(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t.ptr)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dims(shape, role):
    N, narrow, wide, HW = shape
    return (N, narrow, wide, HW) if role == "expand" else (N, wide, narrow, HW)   # N, Cin, Cout, HW


def xf_consts(Cin):
    c = np.arange(Cin)
    scale = np.array([2.0, 4.0, 8.0], np.float32)[c % 3]
    mean = np.array([-0.25, 0.0, 0.5, 0.25], np.float32)[c % 4]
    shift = np.array([0.5, 3.0, 5.5, -1.5, 2.25], np.float32)[c % 5]
    return scale, shift, mean


_REF = {}


def reference(ora, shape, role, dtype):
    """x, dy (rounded to dtype), the transform, dw of the plain read and dw of the transformed read -- computed once"""
    key = (shape, role, dtype)
    if key not in _REF:
        N, Cin, Cout, HW = dims(shape, role)
        x = rounded(det_uniform((N, Cin, 1, HW), "pws/x%s%s" % (shape, role)), dtype)
        dy = rounded(det_uniform((N, Cout, 1, HW), "pws/dy%s%s" % (shape, role)), dtype)
        scale, shift, mean = xf_consts(Cin)
        sc, sh, mu = (v.reshape(1, Cin, 1, 1) for v in (scale, shift, mean))
        xt = np.minimum(np.maximum((x - mu) * sc + (mu * sc + sh), np.float32(0)), np.float32(6)).astype(np.float32)
        assert xt.min() == 0 and xt.max() == 6 and ((xt > 0) & (xt < 6)).mean() > 0.2, "the transform must hit all three ranges"
        xt = rounded(xt, dtype)
        w = np.zeros((Cout, Cin, 1, 1), np.float32)
        _, dw = ora.pwconv_bwd(dy, x, w)
        _, dw_xf = ora.pwconv_bwd(dy, xt, w)
        _REF[key] = (x, dy, (scale, shift, mean), dw.reshape(Cout, Cin), dw_xf.reshape(Cout, Cin))
    return _REF[key]


def run(L, xg, dyg, dims_, dtype, xf=None, lead=0):
    """one call on freshly placed operands; returns dw [Cout, Cin] (host) after checking every guard band"""
    N, Cin, Cout, HW = dims_
    px, pdy = place(xg, lead, "in", "x"), place(dyg, lead, "in", "dy")
    pdw = place(torch.empty((Cout, Cin), dtype=torch.float32, device=DEV), 0, "out", "dw")
    ws = workspace(L.ofasr_pwconv_wgrad_workspace(N, Cin, Cout, HW), DEV)
    if xf is None:
        rc = L.ofasr_pwconv_wgrad(ptr(pdy), ptr(px), ptr(pdw), Cin, N, Cin, Cout, HW, CODE[dtype], ptr(ws), ws.nbytes, stream())
    else:
        rc = L.ofasr_debug_pwconv_wgrad_xf(ptr(pdy), ptr(px), ptr(pdw), Cin, N, Cin, Cout, HW, CODE[dtype], ptr(xf[0]),
                                           ptr(xf[1]), ptr(xf[2]), ptr(ws), ws.nbytes, stream())
    assert rc == 0, "wgrad returned %d (%s)" % (rc, L.ofasr_last_error_string().decode())
    torch.cuda.synchronize()
    for p in (px, pdy, pdw, ws):
        check(p)
    assert not bool(pdw.placement.unwritten().any()), "dw: elements never written"
    return pdw.detach().cpu().numpy().copy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_%dx%d_hw%d" % s)
@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_stream_wgrad_vs_oracle(L, ora, shape, role, dtype):
    C = amd("_C")
    d = dims(shape, role)
    N, Cin, Cout, HW = d
    x, dy, consts, dw_ref, dw_xf_ref = reference(ora, shape, role, dtype)
    xg, dyg = G(x, dtype).view(N, Cin, HW), G(dy, dtype).view(N, Cout, HW)
    xf = tuple(G(v) for v in consts)
    bar = dict(rtol=1e-4, atol=2e-6 * max(1.0, float(np.sqrt(N * HW))))   # test_pwconv_vs_oracle, "dw"
    T = TNAME[dtype]
    variant = 2 if role == "expand" else 1   # the transformed x is the narrow (S) operand of an expand, the wide (R) one of a project

    C.reset_launch_counts()
    got = run(L, xg, dyg, d, dtype)
    assert C.launch_count("pw_wgrad_direct_kernel") == 1 and C.launch_count("pw_wgrad_direct_kernel<%s, 0>" % T) == 1, C.launch_table()
    assert C.launch_count("pw_wgrad_kernel") == 0, C.launch_table()
    print("%s %s %s plain: max|err| = %g (atol %g)" % (shape, role, dtype, np.abs(got - dw_ref).max(), bar["atol"]))
    assert_close(got, dw_ref, what="dw", **bar)
    again = run(L, xg, dyg, d, dtype)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "dw differs between two runs"

    C.reset_launch_counts()
    got_xf = run(L, xg, dyg, d, dtype, xf)
    assert C.launch_count("pw_wgrad_direct_kernel") == 1 and \
        C.launch_count("pw_wgrad_direct_kernel<%s, %d>" % (T, variant)) == 1, C.launch_table()
    print("%s %s %s transformed: max|err| = %g (atol %g)" % (shape, role, dtype, np.abs(got_xf - dw_xf_ref).max(), bar["atol"]))
    assert_close(got_xf, dw_xf_ref, what="dw (transformed x)", **bar)
    again = run(L, xg, dyg, d, dtype, xf)
    assert np.array_equal(got_xf.view(np.uint32), again.view(np.uint32)), "dw (transformed x) differs between two runs"


@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_misaligned_pair_keeps_its_kernel(L, ora, role, dtype):
    """both operands 2 bytes past a 16-byte boundary: no 16-byte access is legal, the call is served as before by the
    staged kernel with scalar loads, and gives the same values (same bar; another summation order)"""
    C = amd("_C")
    shape = SHAPES[1]
    d = dims(shape, role)
    N, Cin, Cout, HW = d
    x, dy, _, dw_ref, _ = reference(ora, shape, role, dtype)
    xg, dyg = G(x, dtype).view(N, Cin, HW), G(dy, dtype).view(N, Cout, HW)
    bar = dict(rtol=1e-4, atol=2e-6 * max(1.0, float(np.sqrt(N * HW))))
    C.reset_launch_counts()
    got = run(L, xg, dyg, d, dtype, lead=2)
    assert C.launch_count("pw_wgrad_direct_kernel") == 0, C.launch_table()
    assert C.launch_count("pw_wgrad_kernel<%s, false>" % TNAME[dtype]) == 1, C.launch_table()
    assert_close(got, dw_ref, what="dw", **bar)
    streamed = run(L, xg, dyg, d, dtype)
    assert_close(got, streamed, what="dw against the aligned call", **bar)


def _all_gradients(L, dtype=BF16):
    """{name: dw} of every shape and role, plain and transformed, on allocator pointers (no oracle)"""
    out = {}
    for shape in SHAPES:
        for role in ROLES:
            N, Cin, Cout, HW = d = dims(shape, role)
            x = det_uniform((N, Cin, 1, HW), "pws/x%s%s" % (shape, role))
            dy = det_uniform((N, Cout, 1, HW), "pws/dy%s%s" % (shape, role))
            xg, dyg = G(x, dtype).view(N, Cin, HW), G(dy, dtype).view(N, Cout, HW)
            xf = tuple(G(v) for v in xf_consts(Cin))
            key = "N%d_%dx%d_hw%d_%s" % (shape + (role,))
            out[key] = run(L, xg, dyg, d, dtype)
            out[key + "_xf"] = run(L, xg, dyg, d, dtype, xf)
    return out


def test_stream_sums_are_the_per_lane_body_sums_bit_for_bit(L, tmp_path):
    """The streaming body keeps the split ranges, the k-slot <-> pixel map and the MFMA chain of the per-lane-load body,
    and with paired splits the first addition of the reduce launch: every gradient equals, bit for bit, what a fresh
    process with OFASR_PW_WGRAD_STREAM=0 (the per-lane-load body; the switch is read once per process) computes."""
    import os
    import subprocess
    import sys
    out = str(tmp_path / "per_lane.npz")
    env = dict(os.environ, OFASR_PW_WGRAD_STREAM="0")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), out], env=env, cwd=os.path.dirname(os.path.abspath(__file__)))
    want = np.load(out)
    got = _all_gradients(L)
    assert sorted(want.files) == sorted(got)
    for k in sorted(got):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), \
            "%s: %d of %d elements differ, max |d| = %g" % (k, int((got[k] != want[k]).sum()), got[k].size,
                                                           float(np.abs(got[k] - want[k]).max()))


def test_flagship_plans_at_most_128_slabs(L):
    """N = 16, 64 <-> 384 channels at 64 x 64: the split-K workspace holds at most 128 slabs of 384 x 64 fp32"""
    for Cin, Cout in ((64, 384), (384, 64)):
        n = L.ofasr_pwconv_wgrad_workspace(16, Cin, Cout, 4096)
        assert 0 < n <= 128 * 384 * 64 * 4, n


if __name__ == "__main__":   # the worker of the bit-for-bit test: every gradient of this process's body -> argv[1] (.npz)
    import sys
    np.savez(sys.argv[1], **_all_gradients(amd("_C").lib()))
