"""--loss / --loss-eps on the two training scripts: what is refused, before anything is set up (no GPU needed).  One
epoch with a fused loss runs in tests/test_hip_losses.py."""
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
def test_loss_eps_without_charbonnier_is_refused(script, tmp_path):
    for extra in ([], ["--loss", "l1"], ["--loss", "mse"], ["--loss", "reference"]):
        r = _run(script, "--path", str(tmp_path), "--synthetic", "--loss-eps", "1e-3", *extra)
        assert r.returncode != 0
        assert "--loss-eps belongs to --loss charbonnier" in r.stdout, r.stdout
        assert not os.listdir(str(tmp_path))                           # refused before anything is set up


@pytest.mark.parametrize("script", SCRIPTS)
def test_a_non_positive_loss_eps_is_refused(script, tmp_path):
    for eps in ("0", "-1e-3", "nan"):
        r = _run(script, "--path", str(tmp_path), "--synthetic", "--loss", "charbonnier", "--loss-eps=" + eps)
        assert r.returncode != 0
        assert "--loss-eps must be positive" in r.stdout, r.stdout
        assert not os.listdir(str(tmp_path))
    r = _run(script, "--path", str(tmp_path), "--loss", "huber")
    assert r.returncode != 0 and "invalid choice" in r.stdout and not os.listdir(str(tmp_path))
