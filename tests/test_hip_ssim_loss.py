"""The SSIM term of the fused training loss on the MI355X (`-m gpu`): ops.sr_loss(ssim=alpha), ofasr_sr_loss_ssim_fwd /
_bwd (csrc/loss.hip) against losses.py, the host statement, and loss_ssim= through both training loops.

Shapes, with T = 16 the kernels' tile edge: [1, 3, 11, 11] is one window per plane; [2, 3, 12, 27] and [1, 3, 27, 61]
make windows and the backward's halo cross tile edges along W alone and along both axes (27 = T + 11: two tiles of
positions, two of pixels; 61 = T + 45: four of each, the last one partial); [3, 3, 64, 64] is whole tiles and several
images.  o takes each dtype; t and s take the other two (MIX).

Bounds.  Forward: S (slot 7) within 1e-9 of the statement, the sum (slot 6) within 1e-9 * K; slots 0, 1, 3, 4 are the
arithmetic of the path without the term: bit for bit what ops.sr_loss(ssim=0) writes for the same operands, and against
the statement as tests/test_hip_losses.py holds them (the two fp64 sums to the summation order, M * 2^-52; the Y-SSE and
its PSNR exactly); slot 2 is the statement's last line on the kernel's own sums, exactly; fp32(L) within one fp32 ulp of
the statement's.  Backward: per element at most 2 ulp of o's dtype at the magnitude of the larger of the pixel addend,
the SSIM addend and the result; the number of differing elements is printed."""
import argparse
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

from conftest import amd
from placed import check_all, lead_of, place

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 16
SHAPES = [(1, 3, 11, 11), (2, 3, 12, T + 11), (1, 3, T + 11, T + 45), (3, 3, 64, 64)]
KINDS = ("mse", "l1", "charbonnier")
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MIX = {"f32": ("f16", "bf16"), "bf16": ("f32", "f16"), "f16": ("bf16", "f32")}     # o's dtype -> (t's, s's)
PREC = {"f32": (24, -126), "f16": (11, -14), "bf16": (8, -126)}     # significand bits, smallest normal exponent
EPS = 1e-3
W = (0.75, 0.5)                                          # w_main, w_kd with a teacher term
ALPHAS = (0.2, 1.0)
sid = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return dict(ops=amd("ops"), losses=amd("losses"), utils=amd("utils"), C=amd("_C"))


def ulp(v, dtype):
    p, emin = PREC[dtype]
    _, e = np.frexp(np.abs(v).astype(np.float64))
    return np.ldexp(1.0, np.maximum(e - 1, emin) - p + 1)


@functools.lru_cache(maxsize=None)
def operands(shape, dtype):
    """(o in `dtype`, t and s in the other two) on the host, made once per (shape, dtype): t an image, o = t blurred a
    little plus noise, values a little outside [0, 1]; some elements of t and s equal o's"""
    g = torch.Generator().manual_seed(1000 * shape[3] + len(dtype))
    t = torch.rand(shape, generator=g).mul_(1.2).sub_(0.1)
    o = (0.5 * t + 0.25 * (t.roll(1, 3) + t.roll(1, 2)) + 0.1 * torch.randn(shape, generator=g)).to(TDT[dtype])
    s = (o.float() + 0.05 * torch.randn(shape, generator=g)).to(TDT[MIX[dtype][1]])
    t = t.to(TDT[MIX[dtype][0]])
    t.view(-1)[::7] = o.to(t.dtype).view(-1)[::7]
    s.view(-1)[::11] = o.to(s.dtype).view(-1)[::11]
    return o, t, s


@functools.lru_cache(maxsize=None)
def ssim_part(shape, dtype):
    """what does not depend on kind, alpha and g: (S, K, dS/do)"""
    losses = amd("losses")
    o, t, _ = operands(shape, dtype)
    on, tn = o.float().numpy(), t.float().numpy()
    S, K = losses.ssim_np(on, tn)
    return S, K, losses.ssim_grad_np(on, tn)


@functools.lru_cache(maxsize=None)
def statement(shape, dtype, kind, with_s, alpha):
    """the host statement for the operands above: the result dict, and per g the (gradient, pixel addend, SSIM addend)"""
    losses = amd("losses")
    o, t, s = operands(shape, dtype)
    on, tn, sn = o.float().numpy(), t.float().numpy(), (s.float().numpy() if with_s else None)
    w_main, w_kd = W if with_s else (1.0, 0.0)
    count = losses.mosaic_count(shape[0], shape[2], shape[3])
    S, K, dS = ssim_part(shape, dtype)
    res = losses.sr_loss_np(on, tn, sn, kind, EPS, w_main, w_kd, psnr_count=count)
    res["ssim"], res["K"] = S, K
    res["loss"] = (1.0 - alpha) * res["loss"] + alpha * (1.0 - S)
    res["loss_f32"] = np.float32(res["loss"])
    grads = {}
    for g in (1.0, 3.0):
        pix = losses.sr_loss_grad_np(on, tn, sn, kind, EPS, (1.0 - alpha) * w_main, (1.0 - alpha) * w_kd, g=g)
        add = (g * -alpha * dS).astype(np.float32)
        grads[g] = (losses.round_to(pix + add, dtype), pix, add)
    return res, grads, count


def test_the_cached_statement_is_the_statement(env):
    """the pieces statement() puts together, against losses.sr_loss_ssim_np / sr_loss_ssim_grad_np called whole"""
    losses = env["losses"]
    shape, dtype = SHAPES[1], "bf16"
    o, t, s = operands(shape, dtype)
    on, tn, sn = o.float().numpy(), t.float().numpy(), s.float().numpy()
    res, grads, count = statement(shape, dtype, "charbonnier", True, 0.2)
    whole = losses.sr_loss_ssim_np(on, tn, sn, "charbonnier", EPS, W[0], W[1], psnr_count=count, alpha=0.2)
    assert whole["loss"] == res["loss"] and whole["ssim"] == res["ssim"] and whole["sum_main"] == res["sum_main"]
    g3 = losses.sr_loss_ssim_grad_np(on, tn, sn, "charbonnier", EPS, W[0], W[1], g=3.0, dtype=dtype, alpha=0.2)
    assert np.array_equal(g3, grads[3.0][0])


def bits(t):
    """the fp32 bit patterns of a tensor's values (16-bit types widen exactly)"""
    return t.detach().float().cpu().numpy().view(np.uint32)


def run(ops, shape, dtype, kind, with_s, alpha, g, placing=None, **kw):
    o, t, s = (x.to(DEV) for x in operands(shape, dtype))
    if placing is not None:
        o = place(o, lead_of(placing[0], o.element_size()), "in", "o")
        t = place(t, lead_of(placing[1], t.element_size()), "in", "t")
        s = place(s, lead_of(placing[2], s.element_size()), "in", "s")
    s = s if with_s else None
    o.requires_grad_(True)
    w_main, w_kd = W if with_s else (1.0, 0.0)
    count = amd("losses").mosaic_count(shape[0], shape[2], shape[3])
    if alpha is not None:
        kw["ssim"] = alpha
    loss, res = ops.sr_loss(o, t, s, kind=kind, eps=EPS, w_main=w_main, w_kd=w_kd, psnr_count=count, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and res.dtype == torch.float64
    (loss if g == 1.0 else loss * 3).backward()
    torch.cuda.synchronize()
    if placing is not None:
        check_all(o, t, s)
    assert o.grad.dtype == o.dtype and o.grad.shape == o.shape
    return loss.detach().cpu(), res.cpu(), o.grad


def check_gradient(grad, want, dtype, what):
    ref, pix, add = want
    got = grad.detach().float().cpu().numpy()
    assert np.isfinite(got).all(), what
    differ = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    mag = np.maximum(np.maximum(np.abs(pix), np.abs(add)), np.abs(ref))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = 2.0 * ulp(mag, dtype)
    print(what, "gradient elements that differ: %d of %d, largest error %.3g ulp" % (
        differ, got.size, float((err / ulp(mag, dtype)).max())))
    assert (err <= bound).all(), "%s: %d elements beyond 2 ulp, worst %.3g ulp" % (
        what, int((err > bound).sum()), float((err / ulp(mag, dtype)).max()))


@pytest.mark.parametrize("with_s", [False, True], ids=["plain", "teacher"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_result_buffer_and_gradient(env, shape, kind, dtype, with_s):
    ops, utils = env["ops"], env["utils"]
    M = float(np.prod(shape))
    w_main, w_kd = W if with_s else (1.0, 0.0)
    _, plain, _ = run(ops, shape, dtype, kind, with_s, None, 1.0)
    for alpha in ALPHAS:
        want, want_g, count = statement(shape, dtype, kind, with_s, alpha)
        for g in (1.0, 3.0):
            what = "%s %s %s %s alpha %g g %g" % (sid(shape), kind, dtype, "teacher" if with_s else "plain", alpha, g)
            loss, res, grad = run(ops, shape, dtype, kind, with_s, alpha, g)
            assert tuple(res.shape) == (8,)
            sa, sb, L, psnr, ssum, S = (float(res[i]) for i in (0, 1, 2, 4, 6, 7))
            sse = int(res.view(torch.int64)[3])
            print(what, "S", S, want["ssim"], "sum", ssum, "loss", L, want["loss"], "sums", sa, want["sum_main"], sb,
                  want["sum_kd"], "sse", sse, want["y_sse"])
            assert abs(S - want["ssim"]) <= 1e-9
            assert abs(ssum - want["ssim"] * want["K"]) <= 1e-9 * want["K"] and S == ssum / want["K"]
            for i in (0, 1, 3, 4):                                  # the arithmetic of the path without the term
                assert res.view(torch.int64)[i] == plain.view(torch.int64)[i], i
            assert abs(sa - want["sum_main"]) <= M * 2.0 ** -52 * want["sum_main"]
            assert abs(sb - want["sum_kd"]) <= M * 2.0 ** -52 * want["sum_kd"]
            assert sse == want["y_sse"] and psnr == utils.psnr_from_sse(sse, count) == want["psnr"]
            assert L == (1.0 - alpha) * (w_main * sa / M + w_kd * sb / M) + alpha * (1.0 - S)
            assert bits(loss)[()] == np.float32(L).view(np.uint32) == int(res.view(torch.int64)[5])
            assert abs(int(bits(loss)[()]) - int(want["loss_f32"].view(np.uint32))) <= 1, (float(loss), want["loss_f32"])
            check_gradient(grad, want_g[g], dtype, what)


def test_equal_operands_score_exactly_one(env):
    ops = env["ops"]
    o = operands(SHAPES[2], "f32")[0].to(DEV).requires_grad_(True)
    loss, res = ops.sr_loss(o, o.detach().clone(), kind="l1", ssim=1.0)
    loss.backward()
    assert float(res[7]) == 1.0 and float(loss) == 0.0 and float(res[6]) == 3.0 * 17 * 51
    assert float(o.grad.abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_two_runs_give_identical_bits(env, shape):
    ops = env["ops"]
    for kind, dtype, with_s, alpha in (("charbonnier", "bf16", True, 0.2), ("l1", "f32", False, 1.0)):
        a = run(ops, shape, dtype, kind, with_s, alpha, 3.0)
        b = run(ops, shape, dtype, kind, with_s, alpha, 3.0)
        assert a[1].numpy().tobytes() == b[1].numpy().tobytes()
        assert a[2].cpu().view(torch.uint8).numpy().tobytes() == b[2].cpu().view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("shape", SHAPES[1:], ids=sid)
def test_without_the_term_nothing_changes(env, shape):
    """ssim=0 and a call without the argument: the kernels of before (launch table), equal bits in loss, buffer, gradient"""
    ops, C = env["ops"], env["C"]
    for kind, dtype, with_s in (("charbonnier", "bf16", True), ("l1", "f32", False), ("mse", "f16", True)):
        C.reset_launch_counts()
        a = run(ops, shape, dtype, kind, with_s, None, 3.0)
        table = C.launch_table()
        assert sum(table.values()) == 3 and not any("ssim" in k for k in table), table
        b = run(ops, shape, dtype, kind, with_s, 0.0, 3.0)
        c = run(ops, shape, dtype, kind, with_s, 0, 3.0, out=torch.empty(6, dtype=torch.float64, device=DEV))
        for x in (b, c):
            assert tuple(x[1].shape) == (6,)
            assert bits(a[0])[()] == bits(x[0])[()] and a[1].numpy().tobytes() == x[1].numpy().tobytes()
            assert a[2].cpu().view(torch.uint8).numpy().tobytes() == x[2].cpu().view(torch.uint8).numpy().tobytes()


def test_launch_counts_and_no_host_sync(env):
    """three launches forward (the stream kernel, the SSIM tile kernel, one fold), one backward; forward and backward
    under torch's sync debug mode, where the installed torch has one"""
    ops, C = env["ops"], env["C"]
    debug = getattr(torch.cuda, "set_sync_debug_mode", lambda mode: None)
    o, t, s = (x.to(DEV) for x in operands(SHAPES[3], "bf16"))
    o.requires_grad_(True)
    out = torch.empty(8, dtype=torch.float64, device=DEV)
    g = torch.full((), 3.0, device=DEV)
    torch.cuda.synchronize()
    C.reset_launch_counts()
    debug("error")
    try:
        loss, res = ops.sr_loss(o, t, s, kind="charbonnier", w_main=W[0], w_kd=W[1], out=out, ssim=0.2)
        fwd = C.launch_table()
        loss.backward(g)
    finally:
        debug("default")
    torch.cuda.synchronize()
    both = C.launch_table()
    assert res is out and sum(fwd.values()) == 3 and sum(both.values()) == 4, both
    for name in ("sr_loss_fwd_kernel", "sr_ssim_fwd_kernel", "sr_loss_ssim_fold_kernel"):
        assert sum(v for k, v in fwd.items() if name in k) == 1, fwd
    assert sum(v for k, v in both.items() if "sr_ssim_bwd_kernel" in k) == 1
    assert bool(torch.isfinite(o.grad.float()).all())
    with pytest.raises(C.OfasrError, match=r"fp64 \[8\]"):
        ops.sr_loss(o, t, out=torch.empty(6, dtype=torch.float64, device=DEV), ssim=0.2)
    with pytest.raises(C.OfasrError, match="fp64"):
        ops.sr_loss(o, t, out=torch.empty(8, dtype=torch.float32, device=DEV), ssim=0.2)


# ------------------------------------------------------------------------------------------------ placement
PLACINGS = [("P1", "P8", "P0"), ("P8", "P1", "P1")]     # o, t, s: odd element offsets, nothing 16-byte aligned but s once


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES[:3], ids=sid)
def test_placed_operands_and_gradient(env, shape, dtype):
    """operands at odd element offsets between NaN bands (a load outside an operand poisons the result), through ops and
    through the C entry point with the gradient and the workspace between guard bands that must stay intact"""
    import placed
    C, ops = env["C"], env["ops"]
    L = C.lib()
    want, want_g, count = statement(shape, dtype, "charbonnier", True, 0.2)
    N, _, H, Wd = shape
    for placing in PLACINGS:
        loss, res, grad = run(ops, shape, dtype, "charbonnier", True, 0.2, 3.0, placing=placing)
        assert abs(float(res[7]) - want["ssim"]) <= 1e-9
        check_gradient(grad, want_g[3.0], dtype, "%s %s placed %s (ops)" % (sid(shape), dtype, placing))
        # ---- the C entry points writing into placed buffers
        o, t, s = (x.to(DEV) for x in operands(shape, dtype))
        po = place(o, lead_of(placing[0], o.element_size()), "in", "o")
        pt = place(t, lead_of(placing[1], t.element_size()), "in", "t")
        ps = place(s, lead_of(placing[2], s.element_size()), "in", "s")
        pres = place(torch.zeros(8, dtype=torch.float64, device=DEV), 8, "out", "result")
        ws = placed.workspace(L.ofasr_sr_loss_ssim_workspace(N, H, Wd), DEV)
        for lead in ("P0", "P1", "P8"):
            pg = place(o, lead_of(lead, o.element_size()), "out", "grad")
            g = torch.full((), 3.0, device=DEV)
            p = lambda x: ctypes.c_void_p(x.data_ptr())
            C.check(L.ofasr_sr_loss_ssim_fwd(p(po), ops._dt(po), p(pt), ops._dt(pt), p(ps), ops._dt(ps), N, H, Wd, 2, EPS,
                                             W[0], W[1], float(count), 0.2, p(pres), ctypes.c_void_p(ws.ptr), ws.nbytes,
                                             ops._stream()), "sr_loss_ssim_fwd")
            C.check(L.ofasr_sr_loss_ssim_bwd(p(po), ops._dt(po), p(pt), ops._dt(pt), p(ps), ops._dt(ps), p(g), N, H, Wd, 2,
                                             EPS, W[0], W[1], 0.2, p(pg), ops._stream()), "sr_loss_ssim_bwd")
            torch.cuda.synchronize()
            check_all(po, pt, ps, pg, pres)
            placed.check(ws)
            assert not bool(pg.placement.unwritten().any())
            assert pres.cpu().numpy().tobytes() == res.numpy().tobytes()
            assert np.array_equal(bits(pg), bits(grad))


_KEEP = []


def _tail(t):
    """a copy of t that ends exactly where its own > 10 MB device allocation ends (the allocator's segment)"""
    nbytes = t.numel() * t.element_size()
    seg = 12 << 20
    torch.cuda.empty_cache()
    # larger than every free block inside a segment that live tensors of earlier tests still pin: the allocator then has
    # to make a new segment of exactly `seg` bytes, whatever ran before
    free = max([b["size"] for s in torch.cuda.memory_snapshot() for b in s["blocks"] if b["state"] == "inactive"] or [0])
    seg = max(seg, (free + (2 << 20) - 1) // (2 << 20) * (2 << 20) + (2 << 20))
    buf = torch.empty(seg, dtype=torch.uint8, device=DEV)
    out = buf[seg - nbytes:].view(t.dtype).view(t.shape)
    out.copy_(t.to(DEV))
    end = out.data_ptr() + nbytes
    segs = [s for s in torch.cuda.memory_snapshot() if s["address"] <= out.data_ptr() < s["address"] + s["total_size"]]
    assert len(segs) == 1 and segs[0]["address"] + segs[0]["total_size"] == end, "tensor is not at its allocation's end"
    _KEEP.append(buf)
    return out


@pytest.mark.parametrize("shape", SHAPES[:3], ids=sid)
def test_operands_that_end_with_their_allocation(env, shape):
    """every operand the tail of an allocation of its own: the planes of the last image end where the memory ends"""
    ops = env["ops"]
    try:
        for dtype in ("bf16", "f32"):
            want, want_g, count = statement(shape, dtype, "l1", True, 0.2)
            o, t, s = (_tail(x) for x in operands(shape, dtype))
            o.requires_grad_(True)
            loss, res = ops.sr_loss(o, t, s, kind="l1", eps=EPS, w_main=W[0], w_kd=W[1], psnr_count=count, ssim=0.2)
            (loss * 3).backward()
            torch.cuda.synchronize()
            assert abs(float(res[7]) - want["ssim"]) <= 1e-9
            check_gradient(o.grad, want_g[3.0], dtype, "%s %s at the end of its allocation" % (sid(shape), dtype))
    finally:
        del _KEEP[:]


# ------------------------------------------------------------------------------------------------ the training loops
class _Teacher(torch.nn.Module):
    """stands in for a teacher network: `scale`-fold nearest upsampling, a little darker"""

    def __init__(self, scale):
        super().__init__()
        self.scale = scale

    def forward(self, x):
        return torch.nn.functional.interpolate(x, scale_factor=self.scale, mode="nearest") * 0.9 if self.scale > 1 else x * 0.9


def _args(**kw):
    a = argparse.Namespace(dynamic_batch_size=2, kd_ratio=0.5, independent_distributed_sampling=False, warmup_epochs=0,
                           warmup_lr=0, validation_frequency=1, teacher_model=None, teacher_path=None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _saved(path):
    ckpt = glob.glob(os.path.join(str(path), "**", "checkpoint.pth.tar"), recursive=True)
    assert len(ckpt) == 1
    return torch.load(ckpt[0], map_location="cpu", weights_only=False)      # written a moment ago by this test


def test_both_training_loops_with_the_term(env, tmp_path):
    rm, nets = amd("imagenet_codebase.run_manager"), amd("elastic_nn.networks")
    ps = amd("elastic_nn.training.progressive_shrinking")
    amd("elastic_nn.modules.dynamic_op").DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    kw = dict(n_epochs=1, init_lr=1e-3, train_batch_size=2, weight_decay=3e-5, no_decay_keys="bn#bias", image_size=32,
              n_train_batches=1)
    net = nets.OFAMobileNetS4(ks_list=[3, 5], expand_ratio_list=[3], depth_list=[2], pixelshuffle_depth_list=[2])
    mgr = rm.SRRunManager(str(tmp_path / "a"), net, rm.SyntheticSRRunConfig(**kw), init=True, num_gpus=1, loss="l1",
                          loss_ssim=0.2)
    first = open(os.path.join(str(tmp_path / "a"), "logs", "train_console.txt")).readline()
    assert first.startswith("Training loss: l1 + 0.2 (1 - SSIM)"), first
    # ---- one step of the teacher loop, one of the progressive-shrinking loop, both with a teacher term
    key = "2x_down_image" if net.active_upscale() == 2 else "4x_down_image"
    loss, psnr = mgr.train_one_epoch(_args(teacher_model=_Teacher(1)), 0, input_key=key)
    assert np.isfinite(loss) and loss > 0 and np.isfinite(psnr)
    s_teacher = mgr.last_train_ssim
    loss, psnr = ps.train_one_epoch(mgr, _args(teacher_model=_Teacher(4)), epoch=0)
    assert np.isfinite(loss) and loss > 0 and np.isfinite(psnr)
    s_shrink = mgr.last_train_ssim
    assert -1.0 <= s_teacher <= 1.0 and -1.0 <= s_shrink <= 1.0 and mgr._ssim_steps == 0
    lines = [l for l in open(os.path.join(str(tmp_path / "a"), "logs", "train_console.txt")) if l.startswith("Train SSIM")]
    assert len(lines) == 2 and "loss calls 1" in lines[0] and "loss calls 2" in lines[1], lines
    assert abs(float(lines[0].split("mean S ")[1].split("\t")[0]) - s_teacher) < 1e-6
    mgr.save_model()
    mgr.save_config()
    saved = _saved(tmp_path / "a")
    assert saved["loss"] == "l1" and saved["loss_ssim"] == 0.2 and "loss_eps" not in saved
    assert '"loss_ssim": 0.2' in open(os.path.join(str(tmp_path / "a"), "run.config")).read()
    # ---- a manager without the term: no such key, no such line
    off = rm.SRRunManager(str(tmp_path / "b"), net, rm.SyntheticSRRunConfig(**kw), init=False, num_gpus=1, loss="l1",
                          loss_ssim=0)
    off.train_one_epoch(_args(teacher_model=_Teacher(1)), 0, input_key=key)
    off.save_model()
    off.save_config()
    assert "loss_ssim" not in _saved(tmp_path / "b") and off.last_train_ssim is None
    text = open(os.path.join(str(tmp_path / "b"), "logs", "train_console.txt")).read()
    assert "SSIM" not in text and text.startswith("Training loss: l1 (fused")
    assert "loss_ssim" not in open(os.path.join(str(tmp_path / "b"), "run.config")).read()
    for bad in (dict(loss="l1", loss_ssim=1.5), dict(loss="l1", loss_ssim=-0.1), dict(loss="reference", loss_ssim=0.2),
                dict(loss_ssim=0.2)):
        with pytest.raises(ValueError, match="loss_ssim"):
            rm.SRRunManager(str(tmp_path / "c"), net, rm.SyntheticSRRunConfig(**kw), init=False, num_gpus=1, **bad)
