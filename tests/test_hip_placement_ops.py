"""The public ops of ops.py on contiguous views that do NOT start where the allocator put them (tests/placed.py).

ops.py allocates its own outputs, so only what the caller hands in is placed: the input x (P1: one element past a
16-byte boundary, P8: 8 bytes past it), a residual, and the upstream gradient handed to backward().  x.contiguous() is a
no-op on such a view, so the kernels see the odd address.  Contract (include/ofasr.h, Conventions): the C ABI may refuse
misalignment where the header says so; ops.py may not -- a caller who passes a contiguous tensor gets a result.

Each op runs once on ordinary tensors and again on placed ones; outputs, input gradients and parameter gradients of the
placed run must match the ordinary run within the tolerance the op already has against its oracle (the aligned and the
unaligned kernels may associate differently), or exactly where both runs take the same kernel by construction (the 16-bit
static conv: ops.py realigns with one clone and the same kernel runs).  The placed inputs must come back untouched, guards
included.
"""
import numpy as np
import pytest
import torch

from conftest import amd, assert_close
from detfill import det_ints, det_uniform
from placed import check, lead_of, place
from test_hip_composite16 import _make_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# what is placed in each re-run: x (and a residual with it) at P1 then P8 with the upstream gradient at P1; then the
# upstream gradient alone
PLACINGS = [("x@P1 dy@P1", "P1", "P1"), ("x@P8 dy@P1", "P8", "P1"), ("dy@P1", None, "P1")]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return amd("ops")


def tol(dtype, scale=1.0):
    """test_hip_kernels.py tol()"""
    if dtype == F32:
        return dict(rtol=2e-5, atol=2e-6 * scale)
    if dtype == BF16:
        return dict(rtol=1e-2, atol=1e-2 * scale)
    return dict(rtol=2e-3, atol=2e-3 * scale)


def wgrad_tol(n_terms):
    """test_hip_kernels.py: weight gradients of the pointwise / depthwise convs"""
    return dict(rtol=1e-4, atol=2e-6 * max(1.0, float(np.sqrt(n_terms))))


def bn_tol(dtype):
    """test_hip_bnact.py _tol()"""
    return {F32: (5e-5, 5e-6), BF16: (1.5e-2, 1.5e-2), F16: (3e-3, 3e-3)}[dtype]


def Hn(t):
    return t.detach().float().cpu().numpy()


def G(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _put(t, where, name):
    return t if where is None else place(t, lead_of(where, t.element_size()), "in", name)


def autograd_run(ops, f, params, reset=None, with_residual=False):
    """run(x, dy, residual) -> {name: tensor} of one forward + backward of f on fresh leaves"""
    def run(x, dy, residual=None):
        if reset is not None:
            reset()
        for p in params:
            p.grad = None
        xr = x.detach().requires_grad_(True)
        assert xr.data_ptr() == x.data_ptr() and xr.is_contiguous()
        rr = residual.detach().requires_grad_(True) if residual is not None else None
        y = f(xr, rr) if with_residual else f(xr)
        out = {"y": y.detach().clone()}
        if dy is not None:
            y.backward(dy)
            ops.flush_deferred()
            out["dx"] = xr.grad.clone()
            if rr is not None:
                out["dresidual"] = rr.grad.clone()
            for i, p in enumerate(params):
                if p.grad is not None:
                    out["dparam%d" % i] = p.grad.clone()
        return out
    return run


def compare(run, x, dy, cmp, residual=None, placings=PLACINGS):
    """the ordinary run, then each placing; cmp(name, got, ref) asserts one tensor.  All failing placings are reported."""
    base = run(x, dy, residual) if residual is not None else run(x, dy)
    errs = []
    for label, wx, wdy in placings:
        if dy is None and wx is None:
            continue
        px = _put(x, wx, "x")
        pr = _put(residual, wx, "residual") if residual is not None else None
        pdy = _put(dy, wdy, "dy") if dy is not None else None
        try:
            got = run(px, pdy, pr) if residual is not None else run(px, pdy)
            torch.cuda.synchronize()
            for p in (px, pr, pdy):
                if p is not None and hasattr(p, "placement"):
                    check(p)
            assert set(got) == set(base), (sorted(got), sorted(base))
            for k in sorted(base):
                cmp(k, got[k], base[k])
        except AssertionError as e:
            errs.append("[%s] %s" % (label, e))
        except Exception as e:      # an op that raises for a placed input: the contract says it may not
            errs.append("[%s] raised %s: %s" % (label, type(e).__name__, e))
    assert not errs, "\n".join(errs)


def close(name, got, ref, rtol, atol):
    assert got.dtype == ref.dtype and got.shape == ref.shape, name
    assert_close(Hn(got), Hn(ref), rtol, atol, name)


# ----------------------------------------------------------------------------------------------- the per-op kernels
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_pwconv_op_placed(ops, dtype):
    N, Cin, Cout, Hh, W = 2, 64, 256, 16, 16
    x = G(det_uniform((N, Cin, Hh, W), "pop/pw/x"), dtype)
    dy = G(det_uniform((N, Cout, Hh, W), "pop/pw/dy"), dtype)
    a = float(np.sqrt(3.0 / Cin))
    w = G(det_uniform((384, Cin, 1, 1), "pop/pw/w", -a, a)).requires_grad_(True)

    def cmp(name, got, ref):
        if name == "y":
            close(name, got, ref, **tol(dtype))
        elif name == "dx":
            close(name, got, ref, **tol(dtype, np.sqrt(Cout / Cin)))
        else:
            close(name, got, ref, **wgrad_tol(N * Hh * W))
    compare(autograd_run(ops, lambda xr: ops.pwconv(xr, w, Cout), [w]), x, dy, cmp)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_dwconv_op_placed(ops, dtype):
    shape, k = (2, 6, 32, 32), 5
    x = G(det_uniform(shape, "pop/dw/x"), dtype)
    dy = G(det_uniform(shape, "pop/dw/dy"), dtype)
    f = G(det_uniform((6, 1, k, k), "pop/dw/f", -0.4, 0.4)).requires_grad_(True)

    def cmp(name, got, ref):
        if name in ("y", "dx"):
            close(name, got, ref, **tol(dtype, k))
        else:
            close(name, got, ref, **wgrad_tol(2 * 32 * 32))
    compare(autograd_run(ops, lambda xr: ops.dwconv(xr, f), [f]), x, dy, cmp)


@pytest.mark.parametrize("res", [False, True], ids=["", "residual"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_bn_act_op_placed(ops, dtype, res):
    shape = (3, 6, 8, 8)
    bn = torch.nn.BatchNorm2d(8).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(G(det_uniform((8,), "pop/bn/g", 0.5, 1.5)))
        bn.bias.copy_(G(det_uniform((8,), "pop/bn/b", -0.3, 0.3)))
    sd0 = {k: v.clone() for k, v in bn.state_dict().items()}
    x = G(det_uniform(shape, "pop/bn/x", -2.0, 2.0), dtype)
    r = G(det_uniform(shape, "pop/bn/r", -1.0, 1.0), dtype) if res else None
    dy = G(det_uniform(shape, "pop/bn/dy"), dtype)
    rt, at = bn_tol(dtype)

    def cmp(name, got, ref):
        if name == "y":
            close(name, got, ref, rt, at)
        elif name == "dx":
            close(name, got, ref, 5 * rt, 5 * at)
        elif name == "dresidual":
            close(name, got, ref, 1e-6, 1e-6)
        else:
            close(name, got, ref, 5 * rt, 20 * at)
    run = autograd_run(ops, (lambda xr, rr: ops.bn_act(xr, bn, ops.ACT_RELU6, rr)) if res else
                       (lambda xr: ops.bn_act(xr, bn, ops.ACT_RELU6)), [bn.weight, bn.bias],
                       reset=lambda: bn.load_state_dict(sd0), with_residual=res)
    compare(run, x, dy, cmp, residual=r)


@pytest.mark.parametrize("dtype", [F32, BF16, torch.int8, torch.float64])
def test_pixel_shuffle_op_placed(ops, dtype):
    """bit-exact, as test_hip_kernels.py test_pixel_shuffle_bit_exact"""
    x = G(det_ints((1, 16, 6, 8), "pop/ps/x", -64, 64)).to(dtype)
    dy = G(det_ints((1, 4, 12, 16), "pop/ps/dy", -64, 64)).to(dtype)

    def cmp(name, got, ref):
        assert torch.equal(got, ref), name
    if dtype.is_floating_point:
        compare(autograd_run(ops, lambda xr: ops.pixel_shuffle(xr, 2), []), x, dy, cmp)
    else:
        compare(lambda xx, _dy: {"y": ops.pixel_shuffle(xx, 2), "back": ops.pixel_unshuffle(ops.pixel_shuffle(xx, 2), 2)},
                x, None, cmp)
    assert torch.equal(ops.pixel_shuffle(x, 2), torch.nn.functional.pixel_shuffle(x, 2))


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_skip_add_op_placed(ops, dtype):
    """one HIP kernel in an inference forward, the same bits as ATen's add; x and skip both placed, then each alone"""
    L = amd("_C")
    x = G(det_uniform((1, 3, 7, 21), "pop/add/x"), dtype)
    s = G(det_uniform((1, 3, 7, 21), "pop/add/s"), dtype)
    ref = x + s
    with torch.no_grad():
        for wx, ws in (("P1", "P1"), ("P8", "P8"), ("P1", None), (None, "P1")):
            px, ps = _put(x, wx, "x"), _put(s, ws, "skip")
            L.reset_launch_counts()
            y = ops.skip_add(px, ps)
            torch.cuda.synchronize()
            assert L.launch_count("add") == 1, L.launch_table()
            for p in (px, ps):
                if hasattr(p, "placement"):
                    check(p)
            assert torch.equal(y, ref), "x@%s skip@%s" % (wx, ws)


# ------------------------------------------------------------------------------------------------ the static ConvLayer
CONV_LAYERS = [(3, 64, 5, "relu6"), (64, 64, 5, "relu6"), (64, 12, 3, "pixelshuffle")]


def _conv_layer(cin, cout, K, act):
    layers = amd("layers")
    layer = layers.ConvLayer(cin, cout, kernel_size=K, use_bn=True, act_func=act).to(DEV)
    tag = "pop/cl/%d_%d_%d" % (cin, cout, K)
    a = float(np.sqrt(3.0 / (cin * K * K)))
    with torch.no_grad():
        layer.conv.weight.copy_(G(det_uniform((cout, cin, K, K), tag + "/w", -a, a)))
        layer.bn.weight.copy_(G(det_uniform((cout,), tag + "/g", 0.5, 1.5)))
        layer.bn.bias.copy_(G(det_uniform((cout,), tag + "/b", -0.5, 0.5)))
        layer.bn.running_mean.copy_(G(det_uniform((cout,), tag + "/rm", -0.2, 0.2)))
        layer.bn.running_var.copy_(G(det_uniform((cout,), tag + "/rv", 0.5, 1.5)))
    return layer


def _conv_cmp(dtype, cin, cout, K, nhw, bn):
    """The 16-bit conv alone: ops.py realigns and the SAME kernel runs -> equality.  With the BatchNorm behind it a placed
    upstream gradient sends the BatchNorm backward to its element-wise kernel, so the layer is compared at the BatchNorm's
    tolerances (test_hip_bnact.py) and its conv weight at the conv's (test_hip_conv2d.py test_conv2d_vs_oracle, 16-bit;
    test_conv2d_fp32_vs_oracle, fp32)."""
    scale = float(np.sqrt(cout * K * K / max(cin * K * K, 1)))
    rt, at = bn_tol(dtype)

    def cmp(name, got, ref):
        if dtype != F32 and not bn:
            assert torch.equal(got, ref), "%s differs although both runs take the same kernel (max |diff| %g)" % (
                name, float((got.float() - ref.float()).abs().max()))
        elif name == "dparam0":      # the conv weight
            if dtype == F32:
                close(name, got, ref, 1e-4, 2e-6 * float(ref.abs().max()) * np.sqrt(nhw))
            else:
                close(name, got, ref, 1e-3, 1e-3 * float(ref.abs().max()))
        elif not bn:
            close(name, got, ref, 5e-5, 5e-6 * (max(1.0, scale) if name == "dx" else 1.0))
        elif name == "y":
            close(name, got, ref, rt, at)
        elif name == "dx":
            close(name, got, ref, 5 * rt, 5 * at)
        else:
            close(name, got, ref, 5 * rt, 20 * at)
    return cmp


@pytest.mark.parametrize("spec", CONV_LAYERS, ids=lambda s: "%dto%d_k%d_%s" % s)
@pytest.mark.parametrize("hw", [(8, 16), (6, 13)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_conv_layer_placed(ops, spec, hw, dtype):
    """ops.conv2d, ops.conv_bn_act_train (ConvLayer in training mode) and ops.conv_bn_act_infer (eval mode, no gradients)
    on placed x / upstream gradients.  6 x 13 is a ragged width, which goes through the pad path."""
    cin, cout, K, act = spec
    Hh, W = hw
    N = 2
    layer = _conv_layer(cin, cout, K, act)
    sd0 = {k: v.clone() for k, v in layer.state_dict().items()}
    reset = lambda: layer.load_state_dict(sd0)
    x = G(det_uniform((N, cin, Hh, W), "pop/cl/x%s%s" % (spec[:3], hw)), dtype)
    oshape = (N, cout // 4, 2 * Hh, 2 * W) if act == "pixelshuffle" else (N, cout, Hh, W)
    dy_conv = G(det_uniform((N, cout, Hh, W), "pop/cl/dyc%s%s" % (spec[:3], hw)), dtype)
    dy_layer = G(det_uniform(oshape, "pop/cl/dyl%s%s" % (spec[:3], hw)), dtype)
    was, ops.CONV_FORCE_HIP = ops.CONV_FORCE_HIP, True
    try:
        compare(autograd_run(ops, lambda xr: ops.conv2d(xr, layer.conv), [layer.conv.weight]), x, dy_conv,
                _conv_cmp(dtype, cin, cout, K, N * Hh * W, False))
        layer.train()
        compare(autograd_run(ops, layer, [layer.conv.weight, layer.bn.weight, layer.bn.bias], reset=reset), x, dy_layer,
                _conv_cmp(dtype, cin, cout, K, N * Hh * W, True))
        layer.eval()
        reset()

        def infer(xx, _dy):
            with torch.no_grad():
                return {"y": layer(xx).clone()}
        compare(infer, x, None, _conv_cmp(dtype, cin, cout, K, N * Hh * W, True))
    finally:
        ops.CONV_FORCE_HIP = was


def test_aligned_input_takes_no_copy(ops):
    """the realignment of a misaligned tensor must cost the aligned case nothing: the same library launches, and the
    tensor the conv saved for its backward IS the caller's (no clone).  A misaligned view is cloned once, to an aligned
    address, and then takes the same launches.  (The library's launch table counts its own kernels; that no copy was made
    is shown by the saved tensor's address.)"""
    C = amd("_C")
    layer = _conv_layer(64, 64, 5, "relu6")
    x = G(det_uniform((2, 64, 8, 16), "pop/nocopy/x"), BF16)
    dy = G(det_uniform((2, 64, 8, 16), "pop/nocopy/dy"), BF16)
    tables = {}
    for label, xx, dd in (("ordinary", x, dy), ("P0", place(x, 0, "in", "x"), place(dy, 0, "in", "dy")),
                          ("P1", place(x, 2, "in", "x"), place(dy, 2, "in", "dy"))):
        layer.conv.weight.grad = None
        xr = xx.detach().requires_grad_(True)
        C.reset_launch_counts()
        y = ops.Conv2dFn.apply(xr, layer.conv.weight)
        saved = y.grad_fn.saved_tensors[0]
        y.backward(dd)
        ops.flush_deferred()
        torch.cuda.synchronize()
        tables[label] = C.launch_table()
        if label == "P1":
            assert saved.data_ptr() != xx.data_ptr() and saved.data_ptr() % 16 == 0
        else:
            assert saved.data_ptr() == xx.data_ptr(), "%s: an aligned input was copied" % label
    assert sum(tables["ordinary"].values()) > 0
    assert tables["P0"] == tables["ordinary"] and tables["P1"] == tables["ordinary"], tables


# --------------------------------------------------------------------------------------------------- the MB block
def _rms(t):
    return float(t.float().pow(2).mean().sqrt()) + 1e-30


def _mb_cmp32():
    """fp32: test_hip_network.py test_mb_block_golden (y 1e-4 / 1e-5, dx 2e-4 / 2e-5, parameters 5e-4 / 2e-5 * max(1,
    max|ref|))"""
    def cmp(name, got, ref):
        if name == "y":
            close(name, got, ref, 1e-4, 1e-5)
        elif name == "dx":
            close(name, got, ref, 2e-4, 2e-5)
        else:
            close(name, got, ref, 5e-4, 2e-5 * max(1.0, float(ref.abs().max())))
    return cmp


def _mb_cmp16(ref32):
    """16-bit: test_hip_bnact.py test_composite_block_matches_per_op_path, the project's bar for two 16-bit realisations
    of one block.  The aligned run forms dy2 and dy1 in registers from (da, y) for their consumer; with a misaligned x or
    upstream gradient the library takes the element-wise kernels, which store each in the activation type first and read
    it back: a different -- not a worse -- realisation.  So both runs are measured against the fp32 run of the same block
    in the L2 norm, and the placed run may be no further from it than 1.25 x the ordinary run's distance + 1e-3 (y, dx) /
    + 2e-3 (parameter gradients), y within 1e-2.  (Measured on MI355X, bf16, K = 3: the two runs are 0.3 % apart on dx and
    dw1 and 1.6 % on BN1's weight gradient, and 4.1 % / 4.8 % / 7.5 % from the block in double, the same to three digits;
    the stage tolerances of test_hip_composite16.py compare a stage with the oracle fed what THAT stage read and do not
    apply to two chains that round in different places.)"""
    def rel(a, r):
        return float((a.double() - r.double()).norm()) / max(float(r.double().norm()), 1e-12)

    def cmp(name, got, base):
        assert got.dtype == base.dtype and got.shape == base.shape and bool(torch.isfinite(got.float()).all()), name
        eg, eb = rel(got, ref32[name]), rel(base, ref32[name])
        bound = 1.25 * eb + (1e-3 if name in ("y", "dx") else 2e-3)
        print("%s: relative L2 distance from the fp32 run: placed %.4g, ordinary %.4g" % (name, eg, eb))
        assert eg <= bound, "%s: placed run %.4g from the fp32 run, ordinary run %.4g (bound %.4g)" % (name, eg, eb, bound)
        if name == "y":
            assert eg <= 1e-2, (name, eg)
    return cmp


def _block(K, train):
    block, layer = _make_block(100 * K + 3)
    block.to(DEV).train(train)
    layer.active_kernel_size, layer.active_expand_ratio = K, 3     # mid = 192
    assert layer.active_middle_channel(64) == 192
    return block, layer


@pytest.mark.parametrize("K", [3, 7])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("entry", ["block", "stack"])
def test_mb_block_training_placed(ops, entry, dtype, K):
    """the composite MB block (ops.FusedMBConvFn through the module, ops.mbstack on the same arguments), training, with the
    identity shortcut: x and the upstream gradient placed.  With only the gradient off, the expand input gradient's
    shortcut addend is the one misaligned pointer."""
    block, layer = _block(K, True)
    sd0 = {k: v.clone() for k, v in block.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 64, 16, 16), generator=g).to(dtype).to(DEV)
    dy = (0.05 * torch.randn((2, 64, 16, 16), generator=g)).to(dtype).to(DEV)
    params = list(block.parameters())
    if entry == "block":
        f = block
    else:
        cfg, ps = layer.composite_args(64, True)
        f = lambda xr: ops.mbstack(xr, [cfg], list(ps))
    was = ops.deferred_weight_grads(True)
    try:
        y = f(x.clone().requires_grad_(True))
        assert type(y.grad_fn).__name__.startswith("FusedMBConvFn" if entry == "block" else "FusedMBStackFn")
        run = autograd_run(ops, f, params, reset=lambda: block.load_state_dict(sd0))
        compare(run, x, dy, _mb_cmp32() if dtype == F32 else _mb_cmp16(run(x.float(), dy.float())))
    finally:
        ops.deferred_weight_grads(was)


@pytest.mark.parametrize("K", [3, 7])
def test_mb_block_inference_placed(ops, K):
    """ops.mbconv_infer (bf16), ops.mbconv_infer_f32 and ops.mbconv_recal_f32 at the same block: x placed.  Tolerances:
    close16 of test_hip_mbfused.py for the 16-bit block; test_hip_recalibrate.py test_recal_block_vs_double for the fp32
    block output (1e-4, 1e-4 * rms) and the accumulated statistics (mean 1e-5 / 2e-5 * sd, variance 2e-4)."""
    block, layer = _block(K, False)
    cfg, ps = layer.composite_args(64, True)
    g = torch.Generator().manual_seed(12)
    x32 = (torch.randn((2, 64, 16, 16), generator=g) + 0.5).to(DEV)
    placings = [("x@P1", "P1", None), ("x@P8", "P8", None)]

    def one(fn):
        def run(xx, _dy):
            with torch.no_grad():
                y = fn(xx)
            assert y is not None, "the kernel declined the block"
            return {"y": y.clone()}
        return run
    compare(one(lambda xx: ops.mbconv_infer(xx, cfg, *ps)), x32.to(BF16), None,
            lambda n, a, b: close(n, a, b, 1e-2, 1e-2 * _rms(b)), placings=placings)
    compare(one(lambda xx: ops.mbconv_infer_f32(xx, cfg, *ps)), x32, None,
            lambda n, a, b: close(n, a, b, 1e-4, 1e-4 * _rms(b)), placings=placings)

    def recal(xx, _dy):
        acc = tuple(torch.zeros((2, c), dtype=torch.float64, device=DEV) for c in (192, 192, 64))
        with torch.no_grad():
            y = ops.mbconv_recal_f32(xx, cfg, *ps, acc=acc)
        assert y is not None, "the kernel declined the block"
        out = {"y": y.clone()}
        for i, a in enumerate(acc):
            out["mean%d" % i], out["var%d" % i] = a[0] / 2, a[1] / 2
        return out
    base = {}

    def cmp(name, got, ref):
        if name == "y":
            close(name, got, ref, 1e-4, 1e-4 * _rms(ref))
        elif name.startswith("mean"):
            sd = np.sqrt(base["var" + name[4:]])
            assert_close(got.cpu().numpy(), ref.cpu().numpy(), 1e-5, 2e-5 * sd + 1e-7, name)
        else:
            base[name] = ref.cpu().numpy()
            assert_close(got.cpu().numpy(), ref.cpu().numpy(), 2e-4, 1e-9, name)
    # variances first (sorted order: "mean*" < "var*" < "y"), so fetch them from an ordinary run up front
    for k_, v_ in recal(x32, None).items():
        if k_.startswith("var"):
            base[k_] = v_.cpu().numpy()
    compare(recal, x32, None, cmp, placings=placings)
