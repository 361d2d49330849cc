"""The --degrade-* options of the two training scripts and of eval_ofa_net_sr.py: every refusal names its option, and
without the options the parsed namespace and the keyword arguments are what they were."""
import argparse
import os
import subprocess
import sys

import pytest

from conftest import ROOT, amd

SCRIPTS = ["train_ofa_net_sr_simple.py", "train_teacher_net_sr_simple.py"]
vf = amd("imagenet_codebase.data_providers.video_frames")


def _parse(*argv):
    ap = argparse.ArgumentParser()
    vf.add_degrade_args(ap)
    return ap.parse_args(list(argv))


def _refused(argv, word, **kw):
    with pytest.raises(SystemExit) as e:
        vf.take_degrade(_parse(*argv), kw.pop("resident", True), **kw)
    assert word in str(e.value), str(e.value)
    return str(e.value)


def test_without_the_options_nothing_is_added():
    a = _parse()
    assert vf.take_degrade(a, False) == {} and a.__dict__ == {}
    assert vf.take_degrade(_parse(), True, {"videos_lr": ["x"]}, "image", "--net x4") == {}


def test_the_spec():
    a = _parse("--degrade-blur", "0.5:3", "--degrade-aniso", "--degrade-noise", "2:25", "--degrade-gray-prob", "0.4",
               "--degrade-prob", "0.9", "--degrade-seed", "77")
    kw = vf.take_degrade(a, True)
    assert a.__dict__ == {}
    assert kw == {"degrade": {"blur": (0.5, 3.0), "aniso": True, "noise": (2.0, 25.0), "gray_prob": 0.4, "prob": 0.9},
                  "degrade_seed": 77}
    kw = vf.take_degrade(_parse("--degrade-noise", "10"), True, {"videos": ["a.y4m"]})
    assert kw == {"degrade": {"blur": (0.0, 0.0), "aniso": False, "noise": (10.0, 10.0), "gray_prob": 0.0, "prob": 1.0},
                  "degrade_seed": 0}


def test_refusals_name_the_option():
    _refused(["--degrade-blur", "1:2"], "--degrade-blur needs --resident or --video", resident=False)
    _refused(["--degrade-noise", "1:2"], "--degrade-noise needs --resident or --video", resident=False)
    _refused(["--degrade-blur", "1:2"], "--degrade-blur with --video-lr", video_kw={"videos": ["a"], "videos_lr": ["b"]})
    msg = _refused(["--degrade-noise", "1:2"], "--degrade-noise: --net x4 takes the HR image", input_key="image",
                   what="--net x4")
    assert "'image'" in msg
    _refused(["--degrade-blur", "2:1"], "--degrade-blur: a range needs 0 <= LO <= HI")
    _refused(["--degrade-blur", "1:4"], "--degrade-blur: HI 4.0 above the limit 3.33333")
    _refused(["--degrade-noise", "1:50.5"], "--degrade-noise: HI 50.5 above the limit 50")
    _refused(["--degrade-noise=-1:5"], "--degrade-noise: a range needs 0 <= LO <= HI")
    _refused(["--degrade-blur", "a:b"], "--degrade-blur takes LO:HI")
    _refused(["--degrade-blur", "1:2:3"], "--degrade-blur takes LO:HI")
    _refused(["--degrade-blur", "1:2", "--degrade-prob", "1.5"], "--degrade-prob: a probability")
    _refused(["--degrade-blur", "1:2", "--degrade-gray-prob", "-0.5"], "--degrade-gray-prob: a probability")
    _refused(["--degrade-noise", "1:2", "--degrade-seed", "-1"], "--degrade-seed must be")
    _refused(["--degrade-aniso"], "--degrade-aniso needs --degrade-blur")
    _refused(["--degrade-noise", "1:2", "--degrade-aniso"], "--degrade-aniso needs --degrade-blur")
    _refused(["--degrade-seed", "3"], "--degrade-seed needs --degrade-blur")
    _refused(["--degrade-prob", "0.5"], "--degrade-prob needs --degrade-blur")
    _refused(["--degrade-gray-prob", "0.5"], "--degrade-gray-prob needs --degrade-blur")


def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True, cwd=ROOT, timeout=900)


@pytest.mark.parametrize("script", SCRIPTS)
def test_the_scripts_refuse_before_anything_is_set_up(script, tmp_path):
    r = _run(script, "--path", str(tmp_path), "--synthetic", "--degrade-blur", "0.5:2")
    assert r.returncode != 0 and "--degrade-blur needs --resident or --video" in r.stdout, r.stdout
    r = _run(script, "--path", str(tmp_path), "--video", "a.y4m", "--video-lr", "b.y4m", "--degrade-noise", "1:5")
    assert r.returncode != 0 and "--degrade-noise with --video-lr" in r.stdout, r.stdout
    assert not os.listdir(str(tmp_path))


def test_net_x4_is_refused(tmp_path):
    r = _run("train_ofa_net_sr_simple.py", "--path", str(tmp_path), "--net", "x4", "--resident", "--degrade-blur", "1:2")
    assert r.returncode != 0 and "--degrade-blur: --net x4 takes the HR image as its input ('image')" in r.stdout, r.stdout
    assert not os.listdir(str(tmp_path))


def test_eval_refuses_bad_values(tmp_path):
    r = _run("eval_ofa_net_sr.py", "--path", str(tmp_path), "--synthetic", "--degrade-blur", "4")
    assert r.returncode != 0 and "--degrade-blur: blur sigma 4.0 outside" in r.stdout, r.stdout
    r = _run("eval_ofa_net_sr.py", "--path", str(tmp_path), "--synthetic", "--degrade-noise", "60")
    assert r.returncode != 0 and "--degrade-noise: noise sigma 60.0 outside" in r.stdout, r.stdout
    r = _run("eval_ofa_net_sr.py", "--path", str(tmp_path), "--synthetic", "--degrade-seed", "3")
    assert r.returncode != 0 and "--degrade-seed needs --degrade-blur" in r.stdout, r.stdout
    assert not os.listdir(str(tmp_path))
