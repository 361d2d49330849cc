"""The scalar BatchNorm rules of csrc/bn_math.h (moments with the variance clamp, invstd / scale / shift, the running
update, the backward coefficients, the ReLU6 clamp and its strict gate, the two backward forms) run on the CPU:
tests/host/bn_math_check.hip is a stand-alone program that walks them over extreme inputs and asserts exact
post-conditions.  It is built with the host sanitizers, so undefined behaviour inside a rule ends it with a non-zero exit
code just as a violated post-condition does.  No GPU, nothing is loaded into this process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
         "-fno-sanitize-recover=undefined"]


def test_bn_rules_hold_on_extreme_inputs(tmp_path):
    exe = str(tmp_path / "bn_math_check")
    build = subprocess.run(["hipcc"] + FLAGS + [os.path.join(HERE, "host", "bn_math_check.hip"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert " 0 failed checks" in run.stdout, run.stdout
