"""The weight EMA of training without a GPU: the host statement (ema.decay_at / update_np / plan_chunks), the refusals of
the three C entry points, --ema-decay / --ema on the command lines, and what --ema makes of a checkpoint.  The kernel and
the trainer run in tests/test_hip_ema.py."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd

TRAINERS = ["train_ofa_net_sr_simple.py", "train_teacher_net_sr_simple.py"]
READERS = [("eval_ofa_net_sr.py", ()), ("search_ofa_net_sr.py", ("--budget-gmacs", "1"))]


# ----------------------------------------------------------------------------------------------------- the definition
def test_decay_warms_up_to_the_option_and_stays():
    ema = amd("ema")
    D = 0.999
    assert ema.decay_at(0, D) == 0.1
    ds = [ema.decay_at(t, D) for t in range(12000)]
    assert all(b >= a for a, b in zip(ds, ds[1:]))
    # (1 + t) / (10 + t) >= D  <=>  t >= (10 D - 1) / (1 - D) = 8990 (up to the rounding of the quotient)
    first = next(t for t, d in enumerate(ds) if d == D)
    assert first in (8989, 8990, 8991), first
    assert first == min(t for t in range(8980, 9000) if (1.0 + t) / (10.0 + t) >= D)
    assert all(d < D for d in ds[:first]) and all(d == D for d in ds[first:])
    assert ema.decay_at(3, 0.2) == 0.2 and ema.decay_at(0, 0.05) == 0.05       # a small D is reached at once
    assert ema.decay_at(1, D) == 2.0 / 11.0


def test_update_np_fixed_points_and_rounding():
    ema = amd("ema")
    rng = np.random.RandomState(0)
    e = rng.standard_normal(4096).astype(np.float32)
    p = rng.standard_normal(4096).astype(np.float32)
    p[::7] = e[::7]
    # w = 1 gives p exactly wherever p - e is exact in fp32 (e + (p - e) then has nothing to round); multiples of 2^-10
    # below 4 are such operands: every difference and sum of two of them fits in 14 bits
    ge = (rng.randint(-4096, 4097, 4096) * 2.0 ** -10).astype(np.float32)
    gp = (rng.randint(-4096, 4097, 4096) * 2.0 ** -10).astype(np.float32)
    assert np.array_equal(ema.update_np(ge, gp, 1.0).view(np.uint32), gp.view(np.uint32))
    assert np.array_equal(ema.update_np(e, p, 0.0).view(np.uint32), e.view(np.uint32))
    for w in (0.0, 2.0 ** -10, np.float32(1 - 0.999), 0.5, 0.9, 1.0):
        assert np.array_equal(ema.update_np(e, e, w).view(np.uint32), e.view(np.uint32))
        got = ema.update_np(e, p, w)
        assert got.dtype == np.float32
        # three fp32 operations, each rounded once: fp64 holds every intermediate exactly before its rounding (a
        # difference or sum of two fp32 values of these magnitudes and a product of two fp32 values fit in 53 bits)
        w32 = np.float64(np.float32(w))
        d = (p.astype(np.float64) - e.astype(np.float64)).astype(np.float32)
        m = (w32 * d.astype(np.float64)).astype(np.float32)
        want = (e.astype(np.float64) + m.astype(np.float64)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), w
        assert np.array_equal(got[::7].view(np.uint32), e[::7].view(np.uint32))
    # the check above tells the statement from a contracted one: with the product left unrounded (what an fma keeps)
    # some of these elements come out differently
    w32 = np.float64(np.float32(0.9))
    d = (p.astype(np.float64) - e.astype(np.float64)).astype(np.float32).astype(np.float64)
    contracted = (e.astype(np.float64) + w32 * d).astype(np.float32)
    assert (contracted != ema.update_np(e, p, 0.9)).any()


def test_plan_chunks_covers_every_element_once_in_order():
    ema = amd("ema")
    chunk = int(amd("_C").lib().ofasr_ema_chunk())
    sizes = [1, 0, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
    rows = ema.plan_chunks(sizes, chunk)
    seen = [[] for _ in sizes]
    for i, off, cnt in rows:
        assert 1 <= cnt <= chunk
        assert 0 <= off and off + cnt <= sizes[i]          # inside ONE tensor
        seen[i].extend(range(off, off + cnt))
    for n, s in zip(sizes, seen):
        assert s == list(range(n))                          # every element exactly once, in order
    assert [i for i, _, _ in rows] == sorted(i for i, _, _ in rows)
    assert all(i != 1 for i, _, _ in rows)                  # the zero-size tensor gives no row
    assert len(rows) == 1 + 0 + 1 + 1 + 1 + 2 + 3
    assert ema.plan_chunks([], chunk) == [] and ema.plan_chunks([5], 2) == [(0, 0, 2), (0, 2, 2), (0, 4, 1)]
    with pytest.raises(ValueError):
        ema.plan_chunks([1], 0)


# -------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    C = amd("_C")
    L = C.lib()
    chunk = L.ofasr_ema_chunk()
    assert chunk > 0 and chunk % 4 == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: L.ofasr_last_error_string().decode()
    assert L.ofasr_ema_update(None, 0, 0.5, None) == 0 and L.ofasr_ema_swap(None, 0, None) == 0     # no launch
    assert L.ofasr_ema_update(None, 3, 0.5, None) == -1 and err() == "ofasr_ema_update: null table"
    assert L.ofasr_ema_swap(None, 3, None) == -1 and err() == "ofasr_ema_swap: null table"
    assert L.ofasr_ema_update(p, -1, 0.5, None) == -1 and err() == "ofasr_ema_update: negative row count"
    assert L.ofasr_ema_swap(p, -1, None) == -1 and err() == "ofasr_ema_swap: negative row count"
    for w in (float("nan"), float("inf"), -float("inf"), -0.25, 1.5):
        assert L.ofasr_ema_update(p, 1, w, None) == -1, w
        assert err() == "ofasr_ema_update: weight outside [0, 1]"
    ops = amd("ops")
    with pytest.raises(C.OfasrError):
        ops.ema_update(torch.zeros((1, 3), dtype=torch.int64), 1, 0.5)
    with pytest.raises(C.OfasrError):
        ops.ema_swap(torch.zeros((1, 3), dtype=torch.int64), 1)


def test_param_ema_refuses_what_it_cannot_average():
    ema = amd("ema")
    with pytest.raises(ValueError, match="layer.weight"):
        ema.ParamEMA([("layer.weight", torch.nn.Parameter(torch.zeros(3)))], 0.999)      # not on the GPU
    for bad in (1.0, -0.1, float("nan"), "x"):
        with pytest.raises(ValueError):
            ema.check_decay(bad)
    assert ema.check_decay(0) == 0.0 and ema.check_decay(0.999) == 0.999


# ---------------------------------------------------------------------------------------------------- command lines
def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True, cwd=ROOT, timeout=900)


@pytest.mark.parametrize("script", TRAINERS)
def test_a_decay_outside_the_unit_interval_is_refused(script, tmp_path):
    for d in ("1", "-0.1", "nan"):
        r = _run(script, "--path", str(tmp_path), "--synthetic", "--ema-decay=" + d)
        assert r.returncode != 0
        assert "--ema-decay must lie in [0, 1)" in r.stdout, r.stdout
        assert not os.listdir(str(tmp_path))                           # refused before anything is set up


@pytest.mark.parametrize("script,extra", READERS, ids=[s for s, _ in READERS])
def test_ema_without_a_checkpoint_is_refused(script, extra, tmp_path):
    r = _run(script, "--path", str(tmp_path), "--synthetic", "--ema", *extra)
    assert r.returncode != 0
    assert "--ema needs --checkpoint" in r.stdout, r.stdout
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("script,extra", READERS, ids=[s for s, _ in READERS])
def test_a_checkpoint_without_an_average_is_refused_by_name(script, extra, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    ckpt = str(tmp_path / "plain_checkpoint.pth.tar")
    torch.save({"state_dict": {"w": torch.zeros(2)}, "epoch": 0}, ckpt)
    r = _run(script, "--path", str(out), "--synthetic", "--checkpoint", ckpt, "--ema", *extra)
    assert r.returncode != 0
    assert "plain_checkpoint.pth.tar" in r.stdout and '"ema"' in r.stdout, r.stdout
    assert not os.listdir(str(out))


def test_averaged_state_dict_lays_the_average_over_the_raw_one():
    ema = amd("ema")
    raw = {"a.weight": torch.arange(4.0), "a.bn.running_mean": torch.ones(2), "b.weight": torch.zeros(3)}
    avg = {"a.weight": torch.arange(4.0) + 0.5, "b.weight": torch.ones(3)}
    ckpt = {"state_dict": raw, "ema": {"decay": 0.999, "updates": 7, "state_dict": avg}}
    sd = ema.averaged_state_dict(ckpt)
    assert list(sd) == list(raw)
    assert torch.equal(sd["a.weight"], avg["a.weight"]) and torch.equal(sd["b.weight"], avg["b.weight"])
    assert sd["a.bn.running_mean"] is raw["a.bn.running_mean"]          # buffers are the network's own
    assert torch.equal(raw["a.weight"], torch.arange(4.0))               # the checkpoint is left as it was
    with pytest.raises(ValueError, match="some/file.pth.tar.*\"ema\""):
        ema.averaged_state_dict({"state_dict": raw}, "some/file.pth.tar")
    with pytest.raises(ValueError, match="c.weight"):
        ema.averaged_state_dict(dict(ckpt, ema={"state_dict": {"c.weight": torch.zeros(1)}}))
    with pytest.raises(ValueError, match="b.weight"):
        ema.averaged_state_dict(dict(ckpt, ema={"state_dict": {"b.weight": torch.zeros(4)}}))
    assert math.isclose(ckpt["ema"]["decay"], 0.999)
