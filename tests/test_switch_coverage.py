"""Every environment switch the library reads has a test of its other side.  (No GPU: this compares names only.)

A switch read in csrc/ -- through one of the readers of csrc/launch.h: env_default_on / env_default_off /
env_positive_int("OFASR_...") or the raw env_value -- must have a row in tests/test_hip_switches.py::SWITCHES -- a fresh
process under the switch, checked against the CPU oracle -- or an entry in COVERED_ELSEWHERE naming the test that flips
it, or the reason it changes no result.  A name in either table must still be read by the sources."""
import glob
import os
import re

from conftest import PKG, ROOT

COVERED_ELSEWHERE = {
    "OFASR_PW_WGRAD_STREAM": "test_hip_pw_wgrad_stream.py::test_stream_sums_are_the_per_lane_body_sums_bit_for_bit",
    "OFASR_MBCONV_SIDE_STREAM": "test_hip_determinism.py::test_step_is_bit_reproducible_and_stream_schedule_invariant",
    "OFASR_MBFUSED_SPLIT": "test_hip_mbfused.py (ofasr_debug_mbfused_split, in-process)",
    "OFASR_MBFUSED_TILE": "test_hip_mbfused.py (ofasr_debug_mbfused_tile, in-process)",
    "OFASR_MBCONV_BN_BWD_STAT": "test_hip_composite16.py::test_composite_block_16bit_vs_oracle[bn2sums_in_dgrad-*] "
                                "(ofasr_debug_mbconv_bn_bwd_stat, in-process)",
    "OFASR_SIDE_STREAM_PRIORITY": "scheduling only: the priority of the side stream, no kernel or operand changes",
}


def _names_in_sources():
    names = set()
    files = glob.glob(os.path.join(ROOT, PKG, "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, PKG, "csrc", "*.h"))
    assert len(files) > 20, files
    for f in files:
        names.update(re.findall(r'\benv_(?:default_on|default_off|positive_int|value)\("(OFASR_[A-Z0-9_]+)"', open(f).read()))
    return names


def test_every_switch_has_a_test_of_its_other_side():
    from test_hip_switches import SWITCHES
    in_rows = {name for row in SWITCHES for name in row["env"]}
    read = _names_in_sources()
    assert len(read) >= 20, sorted(read)
    missing = read - in_rows - set(COVERED_ELSEWHERE)
    assert not missing, "no test flips %s: add a row to tests/test_hip_switches.py::SWITCHES" % sorted(missing)
    stale = (in_rows | set(COVERED_ELSEWHERE)) - read
    assert not stale, "%s: no longer read by csrc/" % sorted(stale)
    both = in_rows & set(COVERED_ELSEWHERE)
    assert not both, "%s: listed in both tables" % sorted(both)


def test_tests_named_as_cover_exist():
    for name, where in COVERED_ELSEWHERE.items():
        if not where.startswith("test_"):
            continue
        path = where.split("::")[0].split(" ")[0]
        src = open(os.path.join(ROOT, "tests", path)).read()
        if "::" in where:
            assert ("def %s(" % where.split("::")[1].split("[")[0].split(" ")[0]) in src, (name, where)
        # the test names the switch, or flips it through its debug setter
        setter = re.search(r"\((ofasr_debug_\w+)", where)
        assert name in src or (setter and setter.group(1) in src), (name, where)


def test_rows_have_unique_ids_and_string_environments():
    from test_hip_switches import SWITCHES
    ids = [r["id"] for r in SWITCHES]
    assert len(set(ids)) == len(ids)
    for r in SWITCHES:
        assert r["env"] and all(k.startswith("OFASR_") and isinstance(v, str) for k, v in r["env"].items()), r["id"]
