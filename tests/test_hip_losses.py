"""The fused training loss on the MI355X (`-m gpu`): the kernels of csrc/loss.hip (ops.sr_loss, ofasr_sr_loss_*) against
losses.py, the host statement -- the gradient bit for bit, the sums to the summation order -- on operands placed
misaligned between guard bands (tests/placed.py), and the --loss flag of the two training scripts.

Shapes: [1, 3, 8, 8] is fewer elements than one workgroup and all vector requests when aligned; [2, 3, 37, 53] has odd
planes (no 16-byte alignment survives, every image ends in a partial chunk); [3, 3, 64, 64] is several workgroups and a
real fold.  Every shape runs aligned (the 16-byte kernels where the shape allows them) and with o one element, t 8 bytes
past a 16-byte boundary and s aligned (the element-wise kernels, whatever the shape)."""
import ctypes
import functools
import glob
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd
from placed import check_all, lead_of, place

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 3, 8, 8), (2, 3, 37, 53), (3, 3, 64, 64)]
KINDS = ("mse", "l1", "charbonnier")
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PLACINGS = [("P0", "P0", "P0"), ("P1", "P8", "P0")]     # o, t, s
EPS = 1e-3
W = (0.75, 0.5)                                          # w_main, w_kd with a teacher term


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return dict(ops=amd("ops"), losses=amd("losses"), utils=amd("utils"), C=amd("_C"))


@functools.lru_cache(maxsize=None)
def operands(shape, dtype):
    """(o in `dtype`, t fp32, s bf16) on the host, made once per (shape, dtype): values a little outside [0, 1], some
    elements of t and s equal to o's (d = 0, e = 0)"""
    g = torch.Generator().manual_seed(1000 * shape[2] + len(dtype))
    o = torch.rand(shape, generator=g).mul_(1.2).sub_(0.1).to(TDT[dtype])
    t = torch.rand(shape, generator=g)
    s = (o.float() + 0.05 * torch.randn(shape, generator=g)).to(torch.bfloat16)
    t.view(-1)[::7] = o.float().view(-1)[::7]
    s.view(-1)[::11] = o.to(torch.bfloat16).view(-1)[::11]
    return o, t, s


@functools.lru_cache(maxsize=None)
def statement(shape, dtype, kind, with_s):
    """the host statement for the operands above: the result dict and the gradients for g = 1 and g = 3"""
    losses = amd("losses")
    o, t, s = operands(shape, dtype)
    on, tn, sn = o.float().numpy(), t.numpy(), (s.float().numpy() if with_s else None)
    w_main, w_kd = W if with_s else (1.0, 0.0)
    count = losses.mosaic_count(shape[0], shape[2], shape[3])
    res = losses.sr_loss_np(on, tn, sn, kind, EPS, w_main, w_kd, psnr_count=count)
    grads = {g: losses.sr_loss_grad_np(on, tn, sn, kind, EPS, w_main, w_kd, g=g, dtype=dtype) for g in (1.0, 3.0)}
    return res, grads, count


def bits(t):
    """the fp32 bit patterns of a tensor's values (16-bit types widen exactly)"""
    return t.detach().float().cpu().numpy().view(np.uint32)


def run(ops, shape, dtype, kind, with_s, placing, g):
    o, t, s = operands(shape, dtype)
    po = place(o.to(DEV), lead_of(placing[0], o.element_size()), "in", "o")
    pt = place(t.to(DEV), lead_of(placing[1], 4), "in", "t")
    ps = place(s.to(DEV), lead_of(placing[2], 2), "in", "s") if with_s else None
    po.requires_grad_(True)
    w_main, w_kd = W if with_s else (1.0, 0.0)
    count = statement(shape, dtype, kind, with_s)[2]
    loss, res = ops.sr_loss(po, pt, ps, kind=kind, eps=EPS, w_main=w_main, w_kd=w_kd, psnr_count=count)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and res.dtype == torch.float64 and tuple(res.shape) == (6,)
    (loss if g == 1.0 else loss * 3).backward()
    torch.cuda.synchronize()
    check_all(po, pt, ps)
    assert po.grad.dtype == po.dtype and po.grad.shape == po.shape
    return loss.detach().cpu(), res.cpu(), po.grad


@pytest.mark.parametrize("with_s", [False, True], ids=["plain", "teacher"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradient_bits_and_result_buffer(env, shape, kind, dtype, with_s):
    ops, utils = env["ops"], env["utils"]
    want, want_g, count = statement(shape, dtype, kind, with_s)
    M = float(np.prod(shape))
    w_main, w_kd = W if with_s else (1.0, 0.0)
    for placing in PLACINGS:
        for g in (1.0, 3.0):
            loss, res, grad = run(ops, shape, dtype, kind, with_s, placing, g)
            got, ref = bits(grad), want_g[g].view(np.uint32)
            bad = np.flatnonzero(got.ravel() != ref.ravel())
            assert bad.size == 0, "%d of %d gradient words differ (%s, g = %g), first at %d: %08x for %08x" % (
                bad.size, got.size, placing, g, bad[0], got.ravel()[bad[0]], ref.ravel()[bad[0]])
            sa, sb, L, psnr = float(res[0]), float(res[1]), float(res[2]), float(res[4])
            sse = int(res.view(torch.int64)[3])
            print(shape, kind, dtype, with_s, placing, g, "sums", sa, want["sum_main"], sb, want["sum_kd"], "loss", L,
                  want["loss"], "sse", sse, want["y_sse"], "psnr", repr(psnr), repr(want["psnr"]))
            assert abs(sa - want["sum_main"]) <= M * 2.0 ** -52 * want["sum_main"]
            assert abs(sb - want["sum_kd"]) <= M * 2.0 ** -52 * want["sum_kd"]
            assert sb == 0.0 or with_s
            assert L == w_main * sa / M + w_kd * sb / M                 # the last line, in fp64, on the kernel's sums
            assert abs(L - want["loss"]) <= (M + 8) * 2.0 ** -52 * want["loss"]
            assert bits(loss)[()] == np.float32(L).view(np.uint32) == int(res.view(torch.int64)[5])
            assert sse == want["y_sse"]
            assert psnr == utils.psnr_from_sse(sse, count)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_runs_give_identical_bytes(env, shape):
    ops = env["ops"]
    for kind, dtype, with_s in (("charbonnier", "bf16", True), ("l1", "f32", False)):
        a = run(ops, shape, dtype, kind, with_s, PLACINGS[1], 3.0)
        b = run(ops, shape, dtype, kind, with_s, PLACINGS[1], 3.0)
        assert a[1].numpy().tobytes() == b[1].numpy().tobytes()
        assert a[2].cpu().view(torch.uint8).numpy().tobytes() == b[2].cpu().view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("lead", ["P0", "P1", "P8"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_gradient_written_between_guard_bands(env, shape, dtype, lead):
    """the C entry point writing into a placed gradient: every element written, no byte outside"""
    C, ops = env["C"], env["ops"]
    L = C.lib()
    o, t, s = operands(shape, dtype)
    want = statement(shape, dtype, "charbonnier", True)[1][3.0]
    po, pt, ps = place(o.to(DEV), 0, "in", "o"), place(t.to(DEV), 0, "in", "t"), place(s.to(DEV), 0, "in", "s")
    pg = place(o.to(DEV), lead_of(lead, o.element_size()), "out", "grad")
    g = torch.full((), 3.0, device=DEV)
    N, _, H, Wd = shape
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    C.check(L.ofasr_sr_loss_bwd(p(po), ops._dt(po), p(pt), ops._dt(pt), p(ps), ops._dt(ps), p(g), N, H, Wd, 2, EPS, W[0],
                                W[1], p(pg), ops._stream()), "sr_loss_bwd")
    torch.cuda.synchronize()
    check_all(po, pt, ps, pg)
    assert not bool(pg.placement.unwritten().any())
    assert np.array_equal(bits(pg), want.view(np.uint32))


def test_mse_gradient_against_aten(env):
    """kind = "mse", fp32 output, no teacher term: dL/do beside ATen's MSELoss autograd on the same tensors.  Both sides
    round three times (d, the scale, the product): 6 * 2^-24 < 2^-21 relative per element."""
    ops = env["ops"]
    for shape in SHAPES:
        o, t, _ = operands(shape, "f32")
        a = o.to(DEV).requires_grad_(True)
        b = o.to(DEV).requires_grad_(True)
        td = t.to(DEV)
        loss, _ = ops.sr_loss(a, td, kind="mse")
        ref = torch.nn.MSELoss()(b, td)
        (loss * 3).backward()
        (ref * 3).backward()
        ga, gb = a.grad.double().cpu().numpy(), b.grad.double().cpu().numpy()
        assert (np.abs(ga - gb) <= 2.0 ** -21 * np.abs(gb)).all(), float((np.abs(ga - gb) / np.maximum(np.abs(gb), 1e-300)).max())
        assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * float(ref.detach())   # ATen adds in fp32


def test_no_host_sync(env):
    """forward and backward under torch's sync debug mode, where the installed torch has one"""
    ops = env["ops"]
    debug = getattr(torch.cuda, "set_sync_debug_mode", lambda mode: None)
    o, t, s = (x.to(DEV) for x in operands(SHAPES[2], "bf16"))
    o.requires_grad_(True)
    out = torch.empty(6, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    debug("error")
    try:
        loss, res = ops.sr_loss(o, t, s, kind="charbonnier", w_main=W[0], w_kd=W[1], out=out)
        (loss * 3).backward()
    finally:
        debug("default")
    torch.cuda.synchronize()
    assert res is out and math.isfinite(float(loss.detach())) and bool(torch.isfinite(o.grad.float()).all())
    with pytest.raises(env["C"].OfasrError, match="fp64"):
        ops.sr_loss(o, t, out=torch.empty(6, dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------------------------ the training scripts
def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True, cwd=ROOT, timeout=900)


def _checkpoint(path):
    ckpt = glob.glob(os.path.join(str(path), "**", "checkpoint.pth.tar"), recursive=True)
    assert len(ckpt) == 1
    # written a moment ago by the script under test; SRRunManager.train stores best_acc as a numpy scalar, which the
    # weights-only unpickler does not take
    return torch.load(ckpt[0], map_location="cpu", weights_only=False)


def _logged(path, pattern):
    """the (psnr, loss) of the epoch's line in logs/valid_console.txt"""
    text = open(os.path.join(str(path), "logs", "valid_console.txt")).read()
    m = re.search(pattern, text)
    assert m, text[-2000:]
    return float(m.group(1)), float(m.group(2))


OFA = ("train_ofa_net_sr_simple.py", "--task", "kernel", "--synthetic", "--resident", "--image-size", "32",
       "--n-train-batches", "2", "--n-epochs", "1")
OFA_LINE = r"Train top-1 ([-+.\dinfa]+), Train loss ([-+.\dinfa]+)"


def test_ofa_script_trains_with_charbonnier(tmp_path):
    r = _run(*OFA, "--path", str(tmp_path), "--loss", "charbonnier")
    assert r.returncode == 0, r.stdout[-4000:]
    psnr, loss = _logged(tmp_path, OFA_LINE)
    assert math.isfinite(psnr) and math.isfinite(loss) and loss > 0.0 and psnr > 0.0
    saved = _checkpoint(tmp_path)
    assert saved["loss"] == "charbonnier" and saved["loss_eps"] == 1e-3
    first = open(os.path.join(str(tmp_path), "logs", "train_console.txt")).readline()
    assert first.startswith("Training loss: charbonnier eps 0.001"), first


def test_teacher_script_trains_with_l1(tmp_path):
    r = _run("train_teacher_net_sr_simple.py", "--synthetic", "--resident", "--image-size", "32", "--batch", "4",
             "--n-epochs", "1", "--path", str(tmp_path), "--loss", "l1")
    assert r.returncode == 0, r.stdout[-4000:]
    psnr, loss = _logged(tmp_path, r"Train top-1 ([-+.\dinfa]+)\tloss ([-+.\dinfa]+)")
    assert math.isfinite(psnr) and math.isfinite(loss) and loss > 0.0 and psnr > 0.0
    saved = _checkpoint(tmp_path)
    assert saved["loss"] == "l1" and "loss_eps" not in saved
    assert open(os.path.join(str(tmp_path), "logs", "train_console.txt")).readline().startswith("Training loss: l1")


def test_default_is_the_reference_loss(tmp_path):
    r = _run(*OFA, "--path", str(tmp_path))
    assert r.returncode == 0, r.stdout[-4000:]
    saved = _checkpoint(tmp_path)
    assert "loss" not in saved and "loss_eps" not in saved
    assert "Training loss" not in open(os.path.join(str(tmp_path), "logs", "train_console.txt")).read()
    psnr, loss = _logged(tmp_path, OFA_LINE)
    assert math.isfinite(psnr) and math.isfinite(loss)


def test_reference_is_the_lines_it_replaced(tmp_path):
    """SRRunManager(loss="reference").train_loss on one seeded batch, bit for bit the lines the two loops ran before the
    loss became selectable (copied here), and the fused losses beside them"""
    F = torch.nn.functional
    utils, rm, nets = amd("utils"), amd("imagenet_codebase.run_manager"), amd("elastic_nn.networks")
    cfg = rm.SyntheticSRRunConfig(n_epochs=1, init_lr=1e-3, train_batch_size=2, weight_decay=3e-5, no_decay_keys="bn#bias",
                                  image_size=32)
    net = nets.OFAMobileNetS4(ks_list=[3], expand_ratio_list=[3], depth_list=[2], pixelshuffle_depth_list=[1])
    mgr = rm.SRRunManager(str(tmp_path / "ref"), net, cfg, init=True, num_gpus=1)
    assert mgr.loss == "reference"
    g = torch.Generator().manual_seed(7)
    images = torch.rand(4, 3, 32, 32, generator=g).to(DEV)
    soft = torch.rand(4, 3, 32, 32, generator=g).to(DEV)
    out16 = torch.rand(4, 3, 32, 32, generator=g).to(DEV).to(torch.bfloat16)
    kd = 0.5
    for shrinking in (False, True):
        for sft in (None, soft):
            a = out16.clone().requires_grad_(True)
            loss, psnr, output = mgr.train_loss(a, images, sft, kd, shrinking=shrinking)
            loss.backward()
            # ---- the parent's lines
            b = out16.clone().requires_grad_(True)
            output_ = b.float()
            loss_ = torch.nn.MSELoss()(output_, images)
            if sft is not None:
                if shrinking:
                    loss_ = (kd * F.mse_loss(output_, sft) + loss_) * (2 / (kd + 1))
                else:
                    loss_ = kd * torch.nn.functional.mse_loss(output_, sft) + loss_
            loss_.backward()
            assert bits(loss)[()] == bits(loss_)[()] and np.array_equal(bits(a.grad), bits(b.grad))
            assert output.dtype == torch.float32 and np.array_equal(bits(output), bits(output_))
            if shrinking:
                assert float(psnr) == float(utils.psnr_y_device(output_, images))
            else:
                assert psnr is None
    fused = rm.SRRunManager(str(tmp_path / "fused"), net, cfg, init=False, num_gpus=1, loss="mse")
    a = out16.clone().requires_grad_(True)
    loss, psnr, output = fused.train_loss(a, images, soft, kd, shrinking=True)
    loss.backward()
    assert output is a and a.grad.dtype == torch.bfloat16 and psnr.dtype == torch.float64 and psnr.dim() == 0
    ref = float((kd * F.mse_loss(out16.float(), soft) + F.mse_loss(out16.float(), images)) * (2 / (kd + 1)))
    assert abs(float(loss) - ref) <= 1e-5 * ref
    assert abs(float(psnr) - float(utils.psnr_y_device(out16.float(), images))) < 0.05
    with pytest.raises(ValueError):
        rm.SRRunManager(str(tmp_path / "bad"), net, cfg, init=False, num_gpus=1, loss="huber")
