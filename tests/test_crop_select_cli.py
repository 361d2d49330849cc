"""--crop-candidates on the two training scripts: refused without a resident training set, and one epoch over a resident
(synthetic) pool prints the per-epoch activity line and records K in the checkpoint."""
import glob
import os
import subprocess
import sys

import pytest

from conftest import ROOT

SCRIPTS = ["train_ofa_net_sr_simple.py", "train_teacher_net_sr_simple.py"]


def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True, cwd=ROOT, timeout=900)


@pytest.mark.parametrize("script", SCRIPTS)
def test_candidates_without_a_resident_set_are_refused(script, tmp_path):
    for extra in ([], ["--synthetic"]):
        r = _run(script, "--path", str(tmp_path), "--crop-candidates", "4", *extra)
        assert r.returncode != 0
        assert "--crop-candidates 4 needs --resident or --video" in r.stdout and "resident pool" in r.stdout, r.stdout
        assert not os.listdir(str(tmp_path))                           # refused before anything is set up
    r = _run(script, "--path", str(tmp_path), "--resident", "--crop-candidates", "17")
    assert r.returncode != 0 and "1 .. 16" in r.stdout


@pytest.mark.gpu
def test_one_epoch_prints_the_activity_line(tmp_path):
    import torch
    r = _run("train_ofa_net_sr_simple.py", "--task", "kernel", "--path", str(tmp_path), "--synthetic", "--resident",
             "--crop-candidates", "4", "--n-train-batches", "2", "--n-epochs", "1", "--image-size", "32")
    assert r.returncode == 0, r.stdout[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("Crop selection [1]")]
    assert len(lines) == 1, r.stdout[-4000:]
    f = lines[0].split("\t")
    assert f[1] == "K=4" and f[2] == "crops 32"                        # two batches of 16
    chosen, first = float(f[3].split()[-1]), float(f[4].split()[-1])
    assert chosen >= first > 0.0                                       # the images are half flat, half noise
    ckpt = glob.glob(os.path.join(str(tmp_path), "**", "checkpoint.pth.tar"), recursive=True)
    assert len(ckpt) == 1
    saved = torch.load(ckpt[0], map_location="cpu", weights_only=True)
    assert saved["crop_candidates"] == 4 and "synthetic_sr" in saved["dataset"]
