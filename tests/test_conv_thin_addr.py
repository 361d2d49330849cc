"""The work split and the global addresses of the thin-side convolutions (csrc/conv_thin_addr.h) run on the CPU:
tests/host/conv_thin_addr_check.hip is a stand-alone program that walks the kernels' own loops -- block, thread, slot,
item -- over a sweep of CU counts, shapes, channel configurations and element sizes and asserts that every request of a
possibly masked lane lies inside its tensor for its full 16 bytes and is aligned, that the segments tile the rows, that
both block mappings are bijections and that the LDS the launchers ask for fits.  Its negative control is the wide request
of the weight gradient as it was before its column clamp covered the lane group's offset: 24, 16 and 8 elements past
the end at W = 8, 16, 24.  Built with the host sanitizers; no GPU, nothing is loaded into this process."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
         "-fno-sanitize-recover=undefined"]


def test_thin_conv_geometry_and_addresses_hold_over_the_sweep(tmp_path):
    exe = str(tmp_path / "conv_thin_addr_check")
    build = subprocess.run(["hipcc"] + FLAGS + [os.path.join(HERE, "host", "conv_thin_addr_check.hip"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert " 0 failed checks" in run.stdout, run.stdout
    # the negative control: the checker sees the old over-read, exactly, and sees none now
    before = dict((int(w), (int(b), int(n))) for w, b, n in re.findall(
        r"wide request before the fix, W=(\d+): (\d+) elements past the end; now: (\d+)", run.stdout))
    assert sorted(before) == [8, 16, 24, 32, 40, 48, 56, 64], run.stdout
    assert [before[w][0] for w in (8, 16, 24)] == [24, 16, 8], run.stdout
    assert all(before[w][0] == 0 for w in (32, 40, 48, 56, 64)), run.stdout
    assert all(n == 0 for _, n in before.values()), run.stdout
