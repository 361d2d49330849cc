"""The weight EMA of training on the MI355X (`-m gpu`): the multi-tensor kernels of csrc/ema.hip against the host statement
(ema.update_np) bit for bit on misaligned, guard-banded operands; one launch and no host read per call; the average inside
both training loops, which it must not disturb; ema_weights() against the inference operand cache and GraphedEval;
checkpoints and resume; the command lines.  The host-side tests are in tests/test_ema.py."""
import argparse
import glob
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd
from placed import check, place, lead_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 0.999
# (parameter lead, shadow lead) per tensor, rotated by the test's parameter: every size meets the vector path (both
# P0), the element path (P1 / P8 on both sides) and a row whose two operands disagree about alignment
PAIRS = [("P0", "P0"), ("P1", "P1"), ("P8", "P8"), ("P0", "P1"), ("P8", "P0"), ("P1", "P8"), ("P0", "P8"), ("P0", "P0"),
         ("P1", "P0")]
WEIGHTS = [1.0, 0.0, 2.0 ** -10, float(np.float32(1 - 0.999)), float(np.float32(0.9))]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    amd("elastic_nn.modules.dynamic_op").DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    C = amd("_C")
    return dict(C=C, L=C.lib(), ops=amd("ops"), ema=amd("ema"), chunk=int(C.lib().ofasr_ema_chunk()),
                rm=amd("imagenet_codebase.run_manager"), nets=amd("elastic_nn.networks"),
                ps=amd("elastic_nn.training.progressive_shrinking"))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]).numpy()


def sizes_of(chunk):
    return [1, 3, 4, 5, 17, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]


def values(sizes, seed):
    """per tensor (p, e): seeded normal draws scaled into 2^-20 <= |x| <= 2^4, a quarter of the elements with p == e.
    p - e is then zero or at least 2^-43 in magnitude, so no subnormal intermediate occurs for the weights used."""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        def draw():
            x = rng.standard_normal(n) * 2.0
            return (np.sign(x) + (x == 0)) * np.clip(np.abs(x), 2.0 ** -20, 2.0 ** 4)
        p, e = draw().astype(np.float32), draw().astype(np.float32)
        same = rng.rand(n) < 0.25
        e[same] = p[same]
        assert (np.abs(p) >= 2.0 ** -20).all() and (np.abs(e) <= 16).all()
        out.append((p, e))
    return out


def placed_operands(env, vals, rot):
    """every p and e between guard bands at its pair's leads, and the kernel's table on the GPU"""
    ps_, es_ = [], []
    for i, (p, e) in enumerate(vals):
        lp, le = PAIRS[(i + 3 * rot) % len(PAIRS)]
        ps_.append(place(torch.from_numpy(p).to(DEV), lead_of(lp, 4), "in", "p%d" % i))
        es_.append(place(torch.from_numpy(e).to(DEV), lead_of(le, 4), "in", "e%d" % i))
    rows = env["ema"].plan_chunks([len(p) for p, _ in vals], env["chunk"])
    host = np.array([[ps_[i].data_ptr() + 4 * off, es_[i].data_ptr() + 4 * off, cnt] for i, off, cnt in rows], dtype=np.int64)
    return ps_, es_, torch.from_numpy(host.reshape(-1, 3)).to(DEV), len(rows)


# ------------------------------------------------------------------------------------------- 1. kernel vs host statement
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_update_is_the_host_statement_bit_for_bit(env, rot):
    sizes = sizes_of(env["chunk"])
    vals = values(sizes, 11 + rot)
    n_elem = sum(sizes)
    for w in WEIGHTS:
        ps_, es_, table, rows = placed_operands(env, vals, rot)
        assert rows == len(sizes) + 1 + 2                      # chunk + 1 gives two rows, 2 chunk + 3 three
        env["ops"].ema_update(table, rows, w, elements=n_elem)
        torch.cuda.synchronize()
        for i, (p, e) in enumerate(vals):
            want = env["ema"].update_np(e, p, w)
            got = es_[i].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (
                "tensor %d (n=%d, leads %s), w=%r: first difference at %d" % (
                    i, sizes[i], PAIRS[(i + 3 * rot) % len(PAIRS)], w,
                    int(np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][0])))
            check(ps_[i])                                        # parameters unchanged byte for byte, guards intact
            check(es_[i], payload=False)                         # the shadow's guards intact
        if w == 0.0:
            for i, (_, e) in enumerate(vals):
                assert np.array_equal(bits(es_[i]), e.view(np.int32))


def test_no_rows_launch_nothing(env):
    C = env["C"]
    table = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    C.reset_launch_counts()
    env["ops"].ema_update(table, 0, 0.5)
    env["ops"].ema_swap(table, 0)
    assert env["L"].ofasr_ema_update(None, 0, 0.5, None) == 0 and env["L"].ofasr_ema_swap(None, 0, None) == 0
    torch.cuda.synchronize()
    assert C.launch_count("ema_kernel") == 0 and not C.launch_table()


# ----------------------------------------------------------------------------------------------------------- 2. swap
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_swap_exchanges_and_twice_restores(env, rot):
    sizes = sizes_of(env["chunk"])
    vals = values(sizes, 23 + rot)
    ps_, es_, table, rows = placed_operands(env, vals, rot)
    env["ops"].ema_swap(table, rows, elements=sum(sizes))
    torch.cuda.synchronize()
    for i, (p, e) in enumerate(vals):
        assert np.array_equal(bits(ps_[i]), e.view(np.int32)), i
        assert np.array_equal(bits(es_[i]), p.view(np.int32)), i
        check(ps_[i], payload=False)
        check(es_[i], payload=False)
    env["ops"].ema_swap(table, rows, elements=sum(sizes))
    torch.cuda.synchronize()
    for i in range(len(vals)):
        check(ps_[i])                                            # as they began, byte for byte, guards intact
        check(es_[i])


# -------------------------------------------------------------------------------------- 3. one launch, no host read
def test_one_launch_and_no_host_sync(env):
    C, ops = env["C"], env["ops"]
    rng = np.random.RandomState(5)
    sizes = [int(n) for n in rng.randint(1, 40, 200)]
    vals = values(sizes, 6)
    w = float(np.float32(1 - 0.999))

    def run():
        ps_ = [torch.from_numpy(p).to(DEV) for p, _ in vals]
        es_ = [torch.from_numpy(e).to(DEV) for _, e in vals]
        rows = env["ema"].plan_chunks(sizes, env["chunk"])
        host = np.array([[ps_[i].data_ptr() + 4 * off, es_[i].data_ptr() + 4 * off, cnt] for i, off, cnt in rows],
                        dtype=np.int64)
        table = torch.from_numpy(host).to(DEV)
        debug = getattr(torch.cuda, "set_sync_debug_mode", lambda mode: None)
        torch.cuda.synchronize()
        C.reset_launch_counts()
        debug("error")
        try:
            ops.ema_update(table, len(rows), w, elements=sum(sizes))
        finally:
            debug("default")
        torch.cuda.synchronize()
        counts = C.launch_table()
        assert sum(counts.values()) == 1 and C.launch_count("ema_kernel") == 1, counts     # 200 tensors, one dispatch
        return [bits(e) for e in es_], ps_

    a, ps_ = run()
    b, _ = run()
    for i, (p, e) in enumerate(vals):
        assert np.array_equal(a[i], b[i])                        # two runs from equal inputs: equal bytes
        assert np.array_equal(a[i], env["ema"].update_np(e, p, w).view(np.int32))
        assert np.array_equal(bits(ps_[i]), p.view(np.int32))


# ---------------------------------------------------------------------------------------------------- 4. in the trainer
def _args(**kw):
    a = argparse.Namespace(dynamic_batch_size=2, kd_ratio=0, independent_distributed_sampling=False, warmup_epochs=0,
                           warmup_lr=0, validation_frequency=1, teacher_model=None, teacher_path=None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


CFG = dict(n_epochs=1, init_lr=1e-3, train_batch_size=2, weight_decay=3e-5, no_decay_keys="bn#bias", image_size=32,
           n_train_batches=2, n_test_batches=2, test_sizes=[32, 40])


def _net(env):
    return env["nets"].OFAMobileNetS4(ks_list=[3], expand_ratio_list=[3], depth_list=[2], pixelshuffle_depth_list=[1])


@pytest.fixture(scope="module")
def start(env):
    """one initial state dict for every manager of this module (CPU tensors, never modified)"""
    torch.manual_seed(3)
    net = _net(env)
    net.init_model("he_fout")
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _manager(env, start, path, ema_decay, **kw):
    net = _net(env)
    net.load_state_dict(start)
    mgr = env["rm"].SRRunManager(str(path), net, env["rm"].SyntheticSRRunConfig(**CFG), init=False, num_gpus=1,
                                 ema_decay=ema_decay, **kw)
    return mgr, net


def _snapshots(mgr, net):
    """wrap step(): the parameters after every optimizer step, as numpy arrays"""
    snaps, inner = [], mgr.step

    def step():
        inner()
        snaps.append([p.detach().cpu().numpy().copy() for p in net.parameters()])
    mgr.step = step
    return snaps


@pytest.mark.parametrize("loop", ["shrinking", "teacher"])
def test_the_average_follows_the_recurrence_and_leaves_training_alone(env, start, tmp_path, loop):
    ema = env["ema"]
    assert ema.weight_at(0, D) == np.float32(0.9) and ema.weight_at(1, D) == np.float32(1 - 2.0 / 11.0)

    def epoch(mgr, net):
        torch.manual_seed(0)                                     # both runs from the same seeds
        if loop == "shrinking":
            return env["ps"].train_one_epoch(mgr, _args(), epoch=0)
        key = "2x_down_image" if net.active_upscale() == 2 else "4x_down_image"
        return mgr.train_one_epoch(_args(), 0, input_key=key)

    mgr, net = _manager(env, start, tmp_path / "on", D)
    shadow = [p.detach().cpu().numpy().copy() for p in net.parameters()]
    first = mgr.ema.state_dict()
    assert first["updates"] == 0 and first["decay"] == D
    for (n, _), s in zip(net.named_parameters(), shadow):       # the shadow starts as a copy of the parameters
        assert np.array_equal(first["state_dict"][n].numpy().view(np.int32), s.view(np.int32))
    snaps = _snapshots(mgr, net)
    result_on = epoch(mgr, net)
    assert len(snaps) == 2 and mgr.ema.updates == 2
    for t, snap in enumerate(snaps):
        shadow = [ema.update_np(e, p, ema.weight_at(t, D)) for e, p in zip(shadow, snap)]
    got = mgr.ema.state_dict()["state_dict"]
    moved = 0
    for (n, _), want in zip(net.named_parameters(), shadow):
        assert np.array_equal(got[n].numpy().view(np.int32), want.view(np.int32)), n
        moved += int(not np.array_equal(want, start[n].numpy()))
    assert moved > 0                                             # the optimizer did move something
    # the same run without the average: every parameter, every buffer and the epoch's result, bit for bit
    off, net_off = _manager(env, start, tmp_path / "off", 0.0)
    assert off.ema is None
    result_off = epoch(off, net_off)
    assert [float(v).hex() for v in result_on] == [float(v).hex() for v in result_off]
    sd_on, sd_off = net.state_dict(), net_off.state_dict()
    for k in sd_on:
        assert torch.equal(sd_on[k], sd_off[k]) and sd_on[k].dtype == sd_off[k].dtype, k
    with pytest.raises(ValueError, match="ema_decay"):
        env["rm"].SRRunManager(str(tmp_path / "bad"), net_off, env["rm"].SyntheticSRRunConfig(**CFG), init=False, num_gpus=1,
                               ema_decay=1.0)


# ---------------------------------------------------------------------------------------------------- 5. the cache trap
def _perturb(net, seed, scale):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((scale * torch.randn(p.shape, generator=g)).to(p.device))


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_ema_weights_get_past_the_operand_cache_and_the_graphs(env, start, tmp_path, prec):
    mgr, net = _manager(env, start, tmp_path / "m", D, mix_prec=prec)
    _perturb(net, 1, 0.05)
    mgr.ema.update()
    mgr.ema.update()
    _perturb(net, 2, 0.05)                                       # the parameters are now well away from the shadow
    net.eval()
    x = torch.rand(2, 3, 24, 20, generator=torch.Generator().manual_seed(9)).to(DEV)

    def forwards(m, n):
        with torch.no_grad():
            with m.autocast():
                plain = n(x)
            return bits(plain), bits(m.graphed(n)(x))

    raw_plain, raw_graph = forwards(mgr, net)
    before = [(p.data_ptr(), bits(p).copy()) for p in net.parameters()]
    # a fresh copy of the network with the averaged parameters loaded from the state dict
    ref_mgr, ref_net = _manager(env, start, tmp_path / "ref", 0.0, mix_prec=prec)
    ref_net.load_state_dict(env["ema"].averaged_state_dict({"state_dict": net.state_dict(), "ema": mgr.ema.state_dict()}))
    ref_net.eval()
    ref_plain, ref_graph = forwards(ref_mgr, ref_net)
    assert not np.array_equal(ref_plain, raw_plain) and not np.array_equal(ref_graph, raw_graph)
    with mgr.ema_weights():
        in_plain, in_graph = forwards(mgr, net)
        avg = mgr.ema.state_dict()["state_dict"]                 # the averaged values, on this side of the swap too
        for n, p in net.named_parameters():
            assert np.array_equal(bits(p), bits(avg[n])), n
    assert np.array_equal(in_plain, ref_plain) and np.array_equal(in_graph, ref_graph)
    assert not np.array_equal(in_plain, raw_plain) and not np.array_equal(in_graph, raw_graph)
    out_plain, out_graph = forwards(mgr, net)
    assert np.array_equal(out_plain, raw_plain) and np.array_equal(out_graph, raw_graph)
    for p, (ptr, b) in zip(net.parameters(), before):
        assert p.data_ptr() == ptr and np.array_equal(bits(p), b)
    with pytest.raises(KeyError):
        with mgr.ema_weights():
            raise KeyError("inside")
    for p, (ptr, b) in zip(net.parameters(), before):            # an exception inside still swaps back
        assert p.data_ptr() == ptr and np.array_equal(bits(p), b)
    assert np.array_equal(forwards(mgr, net)[0], raw_plain)
    with ref_mgr.ema_weights():                                  # a no-op without the average
        assert np.array_equal(forwards(ref_mgr, ref_net)[0], ref_plain)


# ------------------------------------------------------------------------------------------------------ 6. checkpoints
def _load(path, name="checkpoint.pth.tar"):
    # written a moment ago by this test
    return torch.load(os.path.join(str(path), "checkpoint", name), map_location="cpu", weights_only=False)


def _check_ema_entry(entry, net, updates):
    assert type(entry["decay"]) is float and entry["decay"] == D
    assert type(entry["updates"]) is int and entry["updates"] == updates
    names = [n for n, _ in net.named_parameters()]
    assert list(entry["state_dict"]) == names
    for (n, p) in net.named_parameters():
        t = entry["state_dict"][n]
        assert type(t) is torch.Tensor and t.dtype == torch.float32 and t.device.type == "cpu" and t.shape == p.shape


def _one_more_step(mgr, net):
    x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(4)).to(DEV)
    net.train()
    net.set_active_subnet(ks=3, e=3, d=2, pixel_d=1)    # a fresh supernet's active path is not the one last sampled
    mgr.zero_grad()
    with mgr.autocast():
        loss = net(x).float().pow(2).mean()
    loss.backward()
    amd("ops").flush_deferred()
    mgr.step()


def test_checkpoints_carry_the_average_and_resume_exactly(env, start, tmp_path):
    ps = env["ps"]
    mgr, net = _manager(env, start, tmp_path / "a", D)
    log = open(os.path.join(str(tmp_path / "a"), "logs", "train_console.txt")).read().splitlines()
    assert log == ["Weight EMA: decay 0.999 (warm-up (1+t)/(10+t)); validation, best_acc and model_best use the "
                   "averaged weights"]
    ps.train(mgr, _args())
    mgr.save_config()
    assert json.load(open(os.path.join(str(tmp_path / "a"), "run.config")))["ema_decay"] == D
    saved = _load(tmp_path / "a")
    assert saved["ema_decay"] == D
    _check_ema_entry(saved["ema"], net, 2)
    entry_file = str(tmp_path / "entry.pth")
    torch.save(saved["ema"], entry_file)
    torch.load(entry_file, map_location="cpu", weights_only=True)          # tensors, floats, ints and strings only
    for n, p in net.named_parameters():
        assert np.array_equal(bits(saved["state_dict"][n]), bits(p)), n      # the raw weights, as ever
    assert any(not np.array_equal(bits(saved["state_dict"][n]), bits(saved["ema"]["state_dict"][n]))
               for n, _ in net.named_parameters())
    # model_best: the averaged parameters and the network's own buffers
    best = _load(tmp_path / "a", "model_best.pth.tar")["state_dict"]
    assert list(best) == list(saved["state_dict"])
    pnames = {n for n, _ in net.named_parameters()}
    for k, v in best.items():
        want = saved["ema"]["state_dict"][k] if k in pnames else saved["state_dict"][k]
        assert np.array_equal(bits(v.float()), bits(want.float())), k
    # ---- resume: shadow and counter exactly, and one further step as in the uninterrupted run
    mgr.save_model({"epoch": 0, "best_acc": 1.0, "optimizer": mgr.optimizer.state_dict(), "state_dict": net.state_dict()})
    again, net2 = _manager(env, start, tmp_path / "a", D)
    assert again.ema.updates == 0
    again.load_model()
    assert again.ema.updates == 2 and again.start_epoch == 1
    a, b = mgr.ema.state_dict()["state_dict"], again.ema.state_dict()["state_dict"]
    for n in a:
        assert np.array_equal(bits(a[n]), bits(b[n])), n
    _one_more_step(mgr, net)
    _one_more_step(again, net2)
    assert mgr.ema.updates == 3 and again.ema.updates == 3
    a, b = mgr.ema.state_dict()["state_dict"], again.ema.state_dict()["state_dict"]
    for n in a:
        assert np.array_equal(bits(a[n]), bits(b[n])), n
    assert any(not np.array_equal(bits(a[n]), bits(saved["ema"]["state_dict"][n])) for n in a)
    # a stage checkpoint (save_model(model_name=...)) gains the same key
    mgr.save_model(model_name="depth_stage1.pth.tar")
    _check_ema_entry(_load(tmp_path / "a", "depth_stage1.pth.tar")["ema"], net, 3)
    bad = mgr.ema.state_dict()
    bad["state_dict"]["no.such.weight"] = bad["state_dict"].pop(next(iter(bad["state_dict"])))
    with pytest.raises(ValueError, match="no.such.weight"):
        again.ema.load_state_dict(bad)


def test_without_the_option_nothing_changes_and_a_plain_checkpoint_restarts_the_average(env, start, tmp_path):
    off, net = _manager(env, start, tmp_path / "b", 0.0)
    env["ps"].train(off, _args())
    off.save_config()
    saved = _load(tmp_path / "b")
    assert "ema" not in saved and "ema_decay" not in saved
    text = open(os.path.join(str(tmp_path / "b"), "logs", "train_console.txt")).read()
    assert "Weight EMA" not in text
    assert "ema_decay" not in open(os.path.join(str(tmp_path / "b"), "run.config")).read()
    # the same directory, now with the average on: the checkpoint has none, so it starts from the loaded parameters
    on, net_on = _manager(env, start, tmp_path / "b", D)
    on.ema.updates = 5
    on.load_model()
    assert on.ema.updates == 0
    sd = on.ema.state_dict()["state_dict"]
    for n, p in net_on.named_parameters():
        assert np.array_equal(bits(sd[n]), bits(saved["state_dict"][n])), n
    text = open(os.path.join(str(tmp_path / "b"), "logs", "train_console.txt")).read()
    assert re.search(r"Weight EMA: re-initialised from the current parameters, updates = 0 \(.*has no \"ema\" entry\)", text)
    # with the average off an "ema" entry is ignored
    on.save_model({"epoch": 0, "best_acc": 1.0, "optimizer": on.optimizer.state_dict(), "state_dict": net_on.state_dict()})
    assert "ema" in _load(tmp_path / "b")
    off.load_model()
    assert off.ema is None


# ---------------------------------------------------------------------------------------------------------- 7. scripts
def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True, cwd=ROOT, timeout=600)


def _script_checkpoint(path):
    ckpt = glob.glob(os.path.join(str(path), "**", "checkpoint.pth.tar"), recursive=True)
    assert len(ckpt) == 1
    # written a moment ago by the script under test; SRRunManager.train stores best_acc as a numpy scalar, which the
    # weights-only unpickler does not take
    return ckpt[0], torch.load(ckpt[0], map_location="cpu", weights_only=False)


EMA_LINE = "Weight EMA: decay 0.999 (warm-up (1+t)/(10+t)); validation, best_acc and model_best use the averaged weights"
OFA = ("train_ofa_net_sr_simple.py", "--task", "kernel", "--synthetic", "--resident", "--image-size", "32",
       "--n-train-batches", "2", "--n-epochs", "1")


def _check_script_run(path, steps):
    fname, saved = _script_checkpoint(path)
    assert saved["ema_decay"] == D and saved["ema"]["decay"] == D and saved["ema"]["updates"] == steps
    pnames = list(saved["ema"]["state_dict"])
    assert pnames and set(pnames) <= set(saved["state_dict"])
    for n in pnames:
        t = saved["ema"]["state_dict"][n]
        assert t.dtype == torch.float32 and t.shape == saved["state_dict"][n].shape and bool(torch.isfinite(t).all())
    return fname, saved


def test_ofa_script_then_eval_and_export_with_the_average(tmp_path):
    r = _run(*OFA, "--path", str(tmp_path / "train"), "--loss", "l1", "--ema-decay", "0.999")
    assert r.returncode == 0, r.stdout[-4000:]
    lines = open(os.path.join(str(tmp_path / "train"), "logs", "train_console.txt")).read().splitlines()
    assert lines[0].startswith("Training loss: l1") and lines[1] == EMA_LINE, lines[:3]
    fname, saved = _check_script_run(tmp_path / "train", 2)
    assert '"ema_decay": 0.999' in open(os.path.join(str(tmp_path / "train"), "run.config")).read()
    out = str(tmp_path / "export")
    r = _run("eval_ofa_net_sr.py", "--checkpoint", fname, "--ema", "--synthetic", "--depth", "4", "--test-sizes", "64x64,48x80",
             "--path", str(tmp_path / "eval"), "--export", out)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.search(r"Y-PSNR ([-+.\dinfa]+) dB", r.stdout)
    assert m and math.isfinite(float(m.group(1))), r.stdout[-2000:]
    assert json.load(open(os.path.join(out, "net_config.json")))["ema"] is True
    import eval_ofa_net_sr as ev
    ev.load_static(out)                                          # the upscalers' loader takes the export as it is


def test_teacher_script_with_the_average(tmp_path):
    r = _run("train_teacher_net_sr_simple.py", "--synthetic", "--resident", "--image-size", "32", "--batch", "4",
             "--n-epochs", "1", "--path", str(tmp_path), "--ema-decay", "0.999")
    assert r.returncode == 0, r.stdout[-4000:]
    lines = open(os.path.join(str(tmp_path), "logs", "train_console.txt")).read().splitlines()
    assert lines[0] == EMA_LINE, lines[:2]
    fname, saved = _script_checkpoint(tmp_path)
    assert saved["ema_decay"] == D and saved["ema"]["decay"] == D and saved["ema"]["updates"] >= 1
    assert set(saved["ema"]["state_dict"]) <= set(saved["state_dict"])
    best = torch.load(os.path.join(os.path.dirname(fname), "model_best.pth.tar"), map_location="cpu", weights_only=True)
    for n, t in saved["ema"]["state_dict"].items():              # model_best holds the averaged parameters
        assert torch.equal(best["state_dict"][n], t), n
