"""The three thin-side convolution kernels of csrc/conv_thin.hip (ct_out_kernel, ct_in_kernel, ct_wg_kernel + its reduce)
against the fp64 oracle at every launch geometry they have, through the C ABI (include/ofasr.h).

Each kernel picks its work split from the shape and the CU count: column strips (128 wide in 16 bits, 64 in fp32), row
segments of RS = max(8, ceil(H / ceil(CUs / (N * strips)))) rows (ct_in_kernel: at most 64), one of two
blockIdx -> (strip, unit) mappings (N * segs % 8), and for the weight gradient segments of at least ceil(64 / chunks)
rows.  Each part has its own halo, ring-buffer or tail code; the shapes below reach every one of them (what each reaches
is computed from the host rules for 256 CUs and written next to it; test_thin_conv_vs_oracle asserts on the device it
runs on that the multi-segment shapes do get more than one segment).

Operands are placed with tests/placed.py at P0 -- the 16-byte alignment these kernels need -- between NaN guard bands,
inputs must stay unchanged, outputs start as NaN canaries, workspaces have exactly the queried size.  References are
ora.conv2d_fwd / ora.conv2d_bwd on the same rounded inputs (detfill).  Every case runs both layers:
    head (Cin = Cw, Cout = Ct): fwd -> ct_out, dgrad -> ct_in, wgrad role 0;
    stem (Cin = Ct, Cout = Cw): fwd -> ct_in, dgrad -> ct_out with mirrored taps, wgrad role 1;
and after each call the launch table must hold the thin kernel and nothing else.

Tolerances (nothing new; restated from tests/test_hip_conv2d.py):
    16-bit y      rtol = atol = 1e-2 (bf16), 2e-3 (f16)                                 test_conv2d_vs_oracle
    16-bit dx     the same, atol x max(1, sqrt(Cout / Cin))                             test_conv2d_vs_oracle
    16-bit dw     rtol 1e-3, atol 1e-3 * max|dw_ref|                                    test_conv2d_vs_oracle
    fp32 y, dx    rtol 5e-5, atol 5e-6 (dx: x max(1, sqrt(Cout / Cin)))                 test_conv2d_fp32_vs_oracle
    fp32 dw       rtol 1e-4, atol 2e-6 * max|dw_ref| * sqrt(N * H * W)                  test_conv2d_fp32_vs_oracle

The two large-N shapes run the oracle comparison with the light configuration (1, 32, 3) only (tens of millions of
multiply-adds for the CPU oracle); test_row_split_gives_the_same_bits and the statistics test run them at (3, 64, 5)
without an oracle.  No test here places an operand at the end of an allocation: the address rules are checked on the CPU
(tests/test_conv_thin_addr.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd, assert_close
from detfill import det_uniform
from placed import check, place, workspace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CODE = {F32: 0, F16: 1, BF16: 2}
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
OK = 0

# (N, H, W): what it reaches at 256 CUs.  16-bit (strips, segs, RS) of ct_out / ct_in; fp32 strips where they differ; wgrad
# (segs, RS, 32-pixel chunks).
SHAPES = [
    (8, 10, 136),    # (2, 2, 8) strips 128 + 8 (fp32: 3 = 64 + 64 + 8), segments 8 + 2; 16 units: the XCD mapping with > 1 strip; wgrad (1, 10, 5)
    (2, 19, 136),    # (2, 3, 8) segments 8 + 8 + 3; 6 units: the plain mapping with 2 strips; wgrad (2, 13, 5): 13 + 6, last chunk 8 live pixels
    (3, 21, 264),    # (3, 3, 8) 3 strips (fp32: 5), segments 8 + 8 + 5; wgrad (3, 8, 9)
    (1, 13, 72),     # (1, 2, 8) a ragged single strip (fp32: 64 + 8); wgrad (1, 13, 3)
    (2, 19, 128),    # (1, 3, 8) exactly full strips (fp32: 2); wgrad (2, 16, 4): 16 + 3
    (1, 9, 200),     # (2, 2, 8) a last segment of one row (fp32: 4 strips); wgrad (1, 9, 7)
    (1, 1, 8),       # (1, 1, 1) H < K: every halo row outside the image; one item for 8 waves
    (1, 2, 16),      # (1, 1, 2) H < K
    (64, 140, 8),    # (1, 4, 35) a partial 4-row trip in ct_out (35 = 8 * 4 + 3); 256 units; wgrad (3, 64, 1): 64 + 64 + 12
    (128, 132, 8),   # ct_out (1, 2, 66); ct_in capped: (1, 3, 64) = 64 + 64 + 4; wgrad (2, 66, 1)
    (2, 70, 24),     # (1, 9, 8); wgrad (2, 64, 1): one chunk at W = 24 (lane group 3 beyond the row), 64 + 6
    (3, 66, 16),     # (1, 9, 8); wgrad (2, 64, 1): W = 16 (lane groups 2, 3 beyond the row), 64 + 2
    (1, 70, 32),     # (1, 9, 8); wgrad (2, 64, 1): W = 32, every lane group inside, 64 + 6
    (4, 67, 40),     # (1, 9, 8); wgrad (3, 32, 2): a ragged second chunk, 32 + 32 + 3
]
F32_ONLY = (2, 19, 68)   # W % 8 = 4: fwd and dgrad thin (fp32 strips 64 + 4), the weight gradient on the generic fp32 kernel
ONE_SEGMENT = {(1, 1, 8), (1, 2, 16)}
LARGE = {(64, 140, 8), (128, 132, 8)}
EVERY_CONFIG = [(2, 19, 136), (4, 67, 40)]

# (Ct, Cw, K): Ct in 1..4 (the row masks), Cw in {32, 64} (NC = 1, 2; NM = 2, 4; NT = 2, 4), K in {3, 5}, Ct * K <= 16
CONFIGS = [(3, 64, 5), (3, 64, 3), (3, 32, 5), (1, 64, 5), (2, 32, 5), (4, 64, 3), (4, 32, 3), (1, 32, 3)]
LIGHT = (1, 32, 3)


def _cases():
    out = [(s, c) for s in EVERY_CONFIG for c in CONFIGS]
    others = CONFIGS[1:]
    i = 0
    for s in SHAPES + [F32_ONLY]:
        if s in EVERY_CONFIG:
            continue
        if s in LARGE:
            out.append((s, LIGHT))
            continue
        out.append((s, CONFIGS[0]))
        out.append((s, others[i % len(others)]))     # rotated: every configuration meets at least three shapes
        i += 1
    return out


CASES = _cases()
assert all(sum(1 for s, c in CASES if c == cfg) >= 3 for cfg in CONFIGS)
# (dtype, role, case); W % 8 == 4 is an fp32 width (the 16-bit entry points take W % 8 == 0)
PARAMS = [(d, r, c) for d in (BF16, F16, F32) for r in ("head", "stem") for c in CASES if d == F32 or c[0] != F32_ONLY]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return amd("_C").lib()


def tol_y(dtype):
    """test_hip_conv2d.py test_conv2d_vs_oracle / test_conv2d_fp32_vs_oracle: (rtol, atol)"""
    return {BF16: (1e-2, 1e-2), F16: (2e-3, 2e-3), F32: (5e-5, 5e-6)}[dtype]


def rounded(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def G(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def E(shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device=DEV)


def Hn(t):
    return t.detach().float().cpu().numpy()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t.ptr)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def status_ok(L, rc, what):
    assert rc == OK, "%s returned %d (%s)" % (what, rc, L.ofasr_last_error_string().decode())


def finish(*placed_things):
    torch.cuda.synchronize()
    for p in placed_things:
        check(p)


def only_ran(want, what):
    """the launch table holds exactly the kernels of `want` {symbol substring: launches}"""
    C = amd("_C")
    table = C.launch_table()
    for name in table:
        assert any(s in name for s in want), "%s: launched %s; expected only %s (%s)" % (what, name, sorted(want), table)
    for s, n in want.items():
        assert C.launch_count(s) == n, "%s: %d launches of %s, expected %d (%s)" % (what, C.launch_count(s), s, n, table)
    for other in ("conv_igemm_kernel", "conv_wgrad_kernel", "conv_f32_kernel", "conv_f32_wgrad_kernel"):
        if other not in want:
            assert C.launch_count(other) == 0, "%s: %s ran (%s)" % (what, other, table)


def layer(role, cfg):
    Ct, Cw, K = cfg
    return (Cw, Ct, K) if role == "head" else (Ct, Cw, K)      # Cin, Cout, K


def inputs(shape, cfg, role, dtype):
    """x, w, dy: detfill, activations rounded to dtype; w_eff is what the kernel multiplies with"""
    N, Hh, W = shape
    Cin, Cout, K = layer(role, cfg)
    tag = "cthin/%s%s%s" % (shape, cfg, role)
    x = rounded(det_uniform((N, Cin, Hh, W), tag + "/x"), dtype)
    a = float(np.sqrt(3.0 / (Cin * K * K)))
    w = det_uniform((Cout, Cin, K, K), tag + "/w", -a, a)
    dy = rounded(det_uniform((N, Cout, Hh, W), tag + "/dy"), dtype)
    return x, w, dy, (w if dtype == F32 else rounded(w, dtype))


class Conv(object):
    """the seven entry points under one signature; operands placed at P0 between guards, workspaces of the queried size"""

    def __init__(self, L, shape, cfg, role, dtype):
        self.L, self.dtype = L, dtype
        self.N, self.H, self.W = shape
        self.Cin, self.Cout, self.K = layer(role, cfg)
        self.f32 = dtype == F32
        self.dims = (self.N, self.Cin, self.Cout, self.H, self.W, self.K)

    def _ws(self, dgrad):
        L = self.L
        n = L.ofasr_conv2d_f32_workspace(self.Cin, self.Cout, self.K, dgrad) if self.f32 else \
            L.ofasr_conv2d_workspace(self.Cin, self.Cout, self.K, dgrad)
        return workspace(n, DEV)

    def fwd(self, xg, wg, partial_units=None):
        """-> (y, partial or None), all placements checked"""
        L = self.L
        amd("_C").reset_launch_counts()
        px, pw = place(xg, 0, "in", "x"), place(wg, 0, "in", "w")
        py = place(E((self.N, self.Cout, self.H, self.W), self.dtype), 0, "out", "y")
        ws = self._ws(0)
        pp = None
        if partial_units is not None:
            pp = place(E((self.Cout, partial_units, 2)), 0, "out", "partial")
            rc = L.ofasr_conv2d_fwd_stat(ptr(px), ptr(pw), ptr(py), *self.dims, CODE[self.dtype], ptr(pp), partial_units,
                                         ptr(ws), ws.nbytes, stream())
        elif self.f32:
            rc = L.ofasr_conv2d_f32_fwd(ptr(px), ptr(pw), ptr(py), *self.dims, ptr(ws), ws.nbytes, stream())
        else:
            rc = L.ofasr_conv2d_fwd(ptr(px), ptr(pw), ptr(py), *self.dims, CODE[self.dtype], ptr(ws), ws.nbytes, stream())
        status_ok(L, rc, "conv2d fwd")
        finish(*[p for p in (px, pw, py, ws, pp) if p is not None])
        return py, pp

    def dgrad(self, dyg, wg):
        L = self.L
        amd("_C").reset_launch_counts()
        pdy, pw = place(dyg, 0, "in", "dy"), place(wg, 0, "in", "w")
        pdx = place(E((self.N, self.Cin, self.H, self.W), self.dtype), 0, "out", "dx")
        ws = self._ws(1)
        if self.f32:
            rc = L.ofasr_conv2d_f32_dgrad(ptr(pdy), ptr(pw), ptr(pdx), *self.dims, ptr(ws), ws.nbytes, stream())
        else:
            rc = L.ofasr_conv2d_dgrad(ptr(pdy), ptr(pw), ptr(pdx), *self.dims, CODE[self.dtype], ptr(ws), ws.nbytes, stream())
        status_ok(L, rc, "conv2d dgrad")
        finish(pdy, pw, pdx, ws)
        return pdx

    def wgrad(self, dyg, xg):
        L = self.L
        amd("_C").reset_launch_counts()
        pdy, px = place(dyg, 0, "in", "dy"), place(xg, 0, "in", "x")
        pdw = place(E((self.Cout, self.Cin, self.K, self.K)), 0, "out", "dw")
        if self.f32:
            ws = workspace(L.ofasr_conv2d_f32_wgrad_workspace(*self.dims), DEV)
            rc = L.ofasr_conv2d_f32_wgrad(ptr(pdy), ptr(px), ptr(pdw), *self.dims, ptr(ws), ws.nbytes, stream())
        else:
            ws = workspace(L.ofasr_conv2d_wgrad_workspace(*self.dims), DEV)
            rc = L.ofasr_conv2d_wgrad(ptr(pdy), ptr(px), ptr(pdw), *self.dims, CODE[self.dtype], ptr(ws), ws.nbytes, stream())
        status_ok(L, rc, "conv2d wgrad")
        finish(pdy, px, pdw, ws)
        return pdw


def _id(param):
    dtype, role, ((N, Hh, W), (Ct, Cw, K)) = param
    return "%s-%s-%dx%dx%d_t%d_w%d_k%d" % (NAME[dtype], role, N, Hh, W, Ct, Cw, K)


@pytest.mark.parametrize("param", PARAMS, ids=_id)
def test_thin_conv_vs_oracle(L, ora, param):
    dtype, role, (shape, cfg) = param
    N, Hh, W = shape
    Cin, Cout, K = layer(role, cfg)
    x, w, dy, w_eff = inputs(shape, cfg, role, dtype)
    xg, wg, dyg = G(x, dtype), G(w), G(dy, dtype)
    conv = Conv(L, shape, cfg, role, dtype)
    rt, at = tol_y(dtype)
    scale = max(1.0, float(np.sqrt(Cout / Cin)))
    what = "%s %s %s %s" % (role, shape, cfg, NAME[dtype])
    errs = []

    def run(label, fn):
        try:
            fn()
        except AssertionError as e:
            errs.append("[%s %s] %s" % (what, label, e))

    def fwd():
        py, _ = conv.fwd(xg, wg)
        only_ran({"ct_out_kernel" if role == "head" else "ct_in_kernel": 1}, "fwd")
        assert_close(Hn(py), ora.conv2d_fwd(x, w_eff), rt, at, "y")
        if dtype != F32 and shape not in ONE_SEGMENT:
            # the geometry table above is a claim about 256 CUs: on this device the shape must still split its rows
            units = L.ofasr_conv2d_stat_units(N, Cin, Cout, Hh, W, K)
            assert units > N * ((W + 127) // 128), "%d statistics units: one row segment per image on this device" % units

    dx_ref, dw_ref = ora.conv2d_bwd(dy, x, w_eff)      # (dw does not read w)

    def dgrad():
        pdx = conv.dgrad(dyg, wg)
        only_ran({"ct_in_kernel" if role == "head" else "ct_out_kernel": 1}, "dgrad")
        assert_close(Hn(pdx), dx_ref, rt, at * scale, "dx")

    def wgrad():
        pdw = conv.wgrad(dyg, xg)
        if shape == F32_ONLY:
            C = amd("_C")
            assert C.launch_count("ct_wg_kernel") == 0 and C.launch_count("conv_f32_wgrad_kernel") >= 1, \
                "W %% 8 != 0 must take the generic fp32 weight gradient: %s" % (C.launch_table(),)
        else:
            only_ran({"ct_wg_kernel": 1, "ct_wg_reduce_kernel": 1}, "wgrad")
        assert not bool(pdw.placement.unwritten().any()), "dw: elements never written"
        m = float(np.abs(dw_ref).max())
        if dtype == F32:
            assert_close(Hn(pdw), dw_ref, 1e-4, 2e-6 * m * float(np.sqrt(N * Hh * W)), "dw")
        else:
            assert_close(Hn(pdw), dw_ref, 1e-3, 1e-3 * m, "dw")

    run("fwd", fwd)
    run("dgrad", dgrad)
    run("wgrad", wgrad)
    assert not errs, "%d of 3 passes failed:\n%s" % (len(errs), "\n".join(errs))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("role", ["head", "stem"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=lambda d: NAME[d])
def test_row_split_gives_the_same_bits(L, role, dtype):
    """A pixel's operation order in ct_out_kernel and ct_in_kernel does not involve the segment's first row.  Images 0
    and 63 of the (64, 140, 8) batch (RS = 35 at 256 CUs: rows 35, 70, 105 start a segment, the ring is 35 rows deep) are
    computed again alone (N = 1: RS = 8, 18 segments): forward and input gradient must agree bit for bit.  A wrong halo
    or ring row shows exactly, where a tolerance might hide it.  (The weight gradient's slab order does depend on the
    split: it stays at tolerance, above.)"""
    shape, cfg = (64, 140, 8), (3, 64, 5)
    N, Hh, W = shape
    x, w, dy, _ = inputs(shape, cfg, role, dtype)
    wg = G(w)
    batch = Conv(L, shape, cfg, role, dtype)
    alone = Conv(L, (1, Hh, W), cfg, role, dtype)
    y, _ = batch.fwd(G(x, dtype), wg)
    dx = batch.dgrad(G(dy, dtype), wg)
    for n in (0, N - 1):
        y1, _ = alone.fwd(G(x[n:n + 1], dtype), wg)
        only_ran({"ct_out_kernel" if role == "head" else "ct_in_kernel": 1}, "fwd alone")
        dx1 = alone.dgrad(G(dy[n:n + 1], dtype), wg)
        only_ran({"ct_in_kernel" if role == "head" else "ct_out_kernel": 1}, "dgrad alone")
        assert not bool(torch.isnan(y1.float()).any()) and not bool(torch.isnan(dx1.float()).any())
        d = int((_bits(y[n:n + 1]) != _bits(y1)).sum())
        assert d == 0, "%s %s forward, image %d: %d elements differ between the batch and the image alone" % (role, NAME[dtype], n, d)
        d = int((_bits(dx[n:n + 1]) != _bits(dx1)).sum())
        assert d == 0, "%s %s dgrad, image %d: %d elements differ between the batch and the image alone" % (role, NAME[dtype], n, d)


def _rows_per_segment(N, Hh, W, cap):
    """RS of ct_geom / ct_geom_in (csrc/conv_thin_addr.h) for 16-bit elements on this device"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    strips = (W + 127) // 128
    segs = -(-cus // (N * strips))
    RS = -(-Hh // max(segs, 1))
    if RS < 8:
        RS = min(Hh, 8)
    if cap:
        RS = min(RS, 64)
    return strips, -(-Hh // RS), RS


@pytest.mark.parametrize("shape", [(8, 10, 136), (2, 19, 136), (64, 140, 8), (128, 132, 8)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("role", ["head", "stem"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda d: NAME[d])
def test_statistics_epilogue_partials(L, shape, role, dtype):
    """ofasr_conv2d_fwd_stat: every partial[c][p], p < units, is written (NaN canary, guards), and sum_p partial.x /
    partial.y equal the fp64 sum / sum of squares of the output the GPU itself stored, within the worst case of an fp32
    summation of n values in ANY order: n * 2^-24 * sum|v| for the sums, (n + 1) * 2^-24 * sum v^2 for the squares (one
    more rounding for the square itself), n = RS * 128 being the most values one unit holds per channel.  A bound, not a
    measurement."""
    cfg = (3, 64, 5)
    N, Hh, W = shape
    Cin, Cout, K = layer(role, cfg)
    x, w, _, _ = inputs(shape, cfg, role, dtype)
    conv = Conv(L, shape, cfg, role, dtype)
    units = L.ofasr_conv2d_stat_units(N, Cin, Cout, Hh, W, K)
    strips, segs, RS = _rows_per_segment(N, Hh, W, cap=(role == "stem"))
    assert units == N * segs * strips, "units %d; the host rule gives %d x %d x %d" % (units, N, segs, strips)
    assert units > N * strips, "one row segment per image on this device"
    py, pp = conv.fwd(G(x, dtype), G(w), partial_units=units)
    only_ran({"ct_out_kernel" if role == "head" else "ct_in_kernel": 1}, "fwd_stat")
    assert not bool(pp.placement.unwritten().any()), "statistics partials not all written"
    part = pp.cpu().numpy().astype(np.float64)
    assert np.isfinite(part).all()
    yd = py.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(yd).all()
    n = RS * 128
    u = 2.0 ** -24
    s_ref, q_ref = yd.sum(axis=(0, 2, 3)), (yd * yd).sum(axis=(0, 2, 3))
    s_abs = np.abs(yd).sum(axis=(0, 2, 3))
    s_err, q_err = np.abs(part[:, :, 0].sum(axis=1) - s_ref), np.abs(part[:, :, 1].sum(axis=1) - q_ref)
    print("fwd_stat %s %s %s: max sum error / bound %.3g, max square error / bound %.3g"
          % (role, shape, NAME[dtype], float((s_err / (n * u * s_abs)).max()), float((q_err / ((n + 1) * u * q_ref)).max())))
    assert (s_err <= n * u * s_abs).all(), "sum: |error| %s over the bound %s" % (s_err, n * u * s_abs)
    assert (q_err <= (n + 1) * u * q_ref).all(), "sum of squares: |error| %s over the bound %s" % (q_err, (n + 1) * u * q_ref)
