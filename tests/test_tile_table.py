"""The shared table clamps of csrc/tile_table.h (scatter_row, scatter_dest, window_origin, the slab split) run on the CPU:
tests/host/tile_table_check.hip is a stand-alone program that walks them over table rows of extreme values and asserts
the post-conditions every kernel relies on.  It is built with the host sanitizers, so a signed overflow inside a clamp
ends it with a non-zero exit code just as a violated inequality does.  No GPU, nothing is loaded into this process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
         "-fno-sanitize-recover=undefined"]


def test_table_clamps_hold_on_extreme_rows(tmp_path):
    exe = str(tmp_path / "tile_table_check")
    build = subprocess.run(["hipcc"] + FLAGS + [os.path.join(HERE, "host", "tile_table_check.hip"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert " 0 failed checks" in run.stdout, run.stdout
