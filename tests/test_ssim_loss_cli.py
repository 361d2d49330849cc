"""--loss-ssim on the two training scripts: what is refused, before anything is set up (no GPU needed).  One step of each
loop with the SSIM term runs in tests/test_hip_ssim_loss.py."""
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
def test_loss_ssim_with_the_reference_loss_is_refused(script, tmp_path):
    for extra in ([], ["--loss", "reference"]):
        r = _run(script, "--path", str(tmp_path), "--synthetic", "--loss-ssim", "0.2", *extra)
        assert r.returncode != 0
        assert "--loss-ssim belongs to the fused losses" in r.stdout, r.stdout
        assert not os.listdir(str(tmp_path))                           # refused before anything is set up


@pytest.mark.parametrize("script", SCRIPTS)
def test_a_loss_ssim_outside_the_unit_interval_is_refused(script, tmp_path):
    for a in ("1.5", "-0.1"):
        r = _run(script, "--path", str(tmp_path), "--synthetic", "--loss", "l1", "--loss-ssim=" + a)
        assert r.returncode != 0
        assert "--loss-ssim must lie in [0, 1]" in r.stdout, r.stdout
        assert not os.listdir(str(tmp_path))
