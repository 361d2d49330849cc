"""The other side of every kernel switch, against the CPU oracle.

The library picks kernel variants by the OFASR_* environment switches of INTEGRATION.md ("Environment switches, read
once").  A performance change is accepted when the default side beats the switched side in a same-box A/B run
(tools/ab_env.sh); that comparison means something only if both sides compute the same thing.  Each switch is read once
per process, so every row of SWITCHES runs in a fresh child process (this file, started with the row's id) under the
row's environment.  The child runs the row's checks -- the bodies of the existing parity tests, imported, so no tolerance
is restated here -- and asserts from the library's launch counters that the switched kernel served each check.  The
parent runs the same checks under the default environment first (the control, cached between rows) and asserts that the
default kernel served them there: a switch the library silently ignores fails its row.

Children run one at a time (with the parent: two processes on the GPU).  After a child that ended by a signal, by an
abort / fault status or at its time limit, no further child is started.  No row is retried.

tests/test_switch_coverage.py keeps the table complete: every switch csrc/ reads (csrc/launch.h: env_*("OFASR_..."))
has a row here or a named
test elsewhere."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import amd, assert_close

pytestmark = pytest.mark.gpu
HERE = os.path.abspath(__file__)
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
TNAME = {BF16: "ofasr::bf16_t", F16: "ofasr::f16_t", F32: "float"}

# Time limit of a child: 4 x the slowest row measured on the MI355X (9.5 s, pw_wgrad_blocks_1024; the other rows take
# 2.3 - 8.0 s, most of it start-up of the interpreter and the libraries and the oracle's references), rounded up to 10 s.
CHILD_TIMEOUT = 40
FAULT_STATUS = (124, 134, 137, 139)


# ---------------------------------------------------------------------------------------------------- check bodies
# body(ctx, *args) -> the launch table of the call under test (None: the counters as they stand after the body).
# ctx.switched: True in a child (the row's environment), False in the control.
class Ctx(object):
    def __init__(self, switched):
        from oracle import oracle
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        oracle.build()
        self.ora, self.ops, self.C, self.switched = oracle, amd("ops"), amd("_C"), switched
        self.L = self.C.lib()


def body_pw_wgrad(ctx, shape, role, dtype, lead):
    """ofasr_pwconv_wgrad through the C ABI on guard-banded operands, workspace of exactly the queried size (the query
    depends on the switches too): bar of test_hip_kernels.py::test_pwconv_vs_oracle for "dw"; two runs bit-identical"""
    import test_hip_pw_wgrad_stream as ws
    d = N, Cin, Cout, HW = ws.dims(shape, role)
    x, dy, _, dw_ref, _ = ws.reference(ctx.ora, shape, role, dtype)
    xg, dyg = ws.G(x, dtype).view(N, Cin, HW), ws.G(dy, dtype).view(N, Cout, HW)
    bar = dict(rtol=1e-4, atol=2e-6 * max(1.0, float(np.sqrt(N * HW))))
    got = ws.run(ctx.L, xg, dyg, d, dtype, lead=lead)
    table = ctx.C.launch_table()
    print("    max|err| = %g (atol %g)" % (np.abs(got - dw_ref).max(), bar["atol"]))
    assert_close(got, dw_ref, what="dw", **bar)
    again = ws.run(ctx.L, xg, dyg, d, dtype, lead=lead)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "dw differs between two runs"
    return table


def body_pw_wgrad_xf(ctx, shape, role, dtype):
    """the same call with the fused BN + ReLU6 read of x (test_hip_pw_wgrad_stream.py), same bar"""
    import test_hip_pw_wgrad_stream as ws
    d = N, Cin, Cout, HW = ws.dims(shape, role)
    x, dy, consts, _, dw_xf_ref = ws.reference(ctx.ora, shape, role, dtype)
    xg, dyg = ws.G(x, dtype).view(N, Cin, HW), ws.G(dy, dtype).view(N, Cout, HW)
    got = ws.run(ctx.L, xg, dyg, d, dtype, tuple(ws.G(v) for v in consts))
    assert_close(got, dw_xf_ref, what="dw (transformed x)", rtol=1e-4, atol=2e-6 * max(1.0, float(np.sqrt(N * HW))))


def body_pwconv(ctx, case, dtype):
    import test_hip_kernels as tk
    tk.test_pwconv_vs_oracle(ctx.ops, ctx.ora, case, dtype)


def body_dwconv(ctx, shape, k, dtype):
    import test_hip_kernels as tk
    tk.test_dwconv_vs_oracle(ctx.ops, ctx.ora, shape, k, dtype)


def body_bn_bwd(ctx, dtype, training, shape):
    """16-bit BN backward, no activation, no residual: dx, dgamma, dbeta at the bars of test_hip_bnact.py"""
    import test_hip_bnact as tb
    tb.test_bn_bwd_large_shapes(dtype, 0, training, shape)


def body_conv16(ctx, case, dtype):
    import test_hip_conv2d as tc
    tc.test_conv2d_vs_oracle(ctx.ora, case, dtype)


def body_conv32(ctx, case):
    import test_hip_conv2d as tc
    tc.test_conv2d_fp32_vs_oracle(ctx.ora, case)


def body_block(ctx, case, bstat, profile):
    """the composite MB block, stage by stage (test_hip_composite16.py::check_block); the control runs the default
    profile, whose routing assertions are those of the timed path"""
    import test_hip_composite16 as tb
    return tb.check_block(ctx.ora, case, bstat, profile if ctx.switched else tb.DEFAULT_PROFILE)


KT_KERNELS = ("kt_fwd_kernel", "kt_bwd_chain_kernel", "kt_bwd_mat_kernel")


def body_stack(ctx, dtype):
    """test_hip_deferred.py::test_mb_stack_call_equals_block_by_block: bit equality of the stack call and the blocks.
    With OFASR_MBSTACK_KT_BATCH=0 the stack makes the per-block kernel-transform launches of the block-by-block path"""
    import test_hip_deferred as td
    tables = td.check_stack_equals_blocks(dtype)

    def ran(t, part):
        return sum(n for name, n in t.items() if part in name)

    if ctx.switched:
        for k in KT_KERNELS:
            assert ran(tables[True], k) == ran(tables[False], k), (k, tables)
        assert ran(tables[True], "_batch_kernel") == 0, tables[True]
    return tables[True]


BODIES = {f.__name__[5:]: f for f in (body_pw_wgrad, body_pw_wgrad_xf, body_pwconv, body_dwconv, body_bn_bwd, body_conv16,
                                     body_conv32, body_block, body_stack)}


# a switch whose effect no kernel name shows (a split count): a workspace query that must differ from the default's
def probe_pw_wgrad_ws(ctx):
    return [int(ctx.L.ofasr_pwconv_wgrad_workspace(N, 64, 384, 4096)) for N in (16, 64)]


def probe_conv_f32_wg_ws(ctx):
    return [int(ctx.L.ofasr_conv2d_f32_wgrad_workspace(16, 64, 64, 64, 64, 5))]


PROBES = {"pw_wgrad_ws": probe_pw_wgrad_ws, "conv_f32_wg_ws": probe_conv_f32_wg_ws}


# ---------------------------------------------------------------------------------------------------- the table
def chk(body, args, child_must=None, child_never=(), ctrl_must=None, ctrl_never=()):
    """one check of a row.  *_must: {kernel-name substring: launches (None: at least one)} in the launch table of the
    check; *_never: substrings with no launch.  child_*: under the row's environment; ctrl_*: under the default's"""
    return dict(body=body, args=tuple(args), child_must=dict(child_must or {}), child_never=tuple(child_never),
                ctrl_must=dict(ctrl_must or {}), ctrl_never=tuple(ctrl_never))


def swap(body, args, alt, dflt, both=None, never=()):
    """the switched side runs `alt` and not `dflt`, the default side the reverse; `both` / `never` hold on either side"""
    alt, dflt, both = dict(alt), dict(dflt), dict(both or {})
    return chk(body, args, dict(alt, **both), tuple(dflt) + tuple(never), dict(dflt, **both), tuple(alt) + tuple(never))


def _f32_direct_checks():
    shapes = [(1, 64, 384, 64),
              (1, 64, 384, 96),      # three 32-pixel units in one split: the pair loop's odd tail
              (1, 60, 380, 36),      # HW % 4 == 0 but not % 32, NS < 64, MR % 32 != 0, clamped pixel requests
              (3, 64, 256, 100),     # units straddle images; the last unit of an image holds 4 pixels
              (2, 64, 192, 1024)]
    out = [swap("pw_wgrad", (s, role, F32, 0), {"pw_wgrad_direct_f32_kernel": 1}, {"pw_wgrad_kernel": 1})
           for s in shapes for role in ("expand", "project")]
    # 4 bytes past a 16-byte boundary: no vector load is legal, the staged kernel with scalar loads serves both sides
    out += [swap("pw_wgrad", ((1, 64, 384, 96), role, F32, 4), {}, {}, both={"pw_wgrad_kernel<float, false>": 1},
                 never=("pw_wgrad_direct_f32_kernel",)) for role in ("expand", "project")]
    return out


PW_SWITCH_CASES = [(2, 64, 256, 64, 384, 16, 16), (2, 256, 64, 384, 64, 16, 16), (1, 64, 192, 64, 384, 16, 16),
                   (2, 64, 384, 64, 384, 16, 16), (2, 384, 64, 384, 64, 16, 16)]


def _fanout_checks():
    out = []
    for dt in (BF16, F16):
        for case in PW_SWITCH_CASES:
            if case[1:3] == (64, 192):   # 1.5 slabs: the generic fan-out kernel on both sides
                out.append(swap("pwconv", (case, dt), {}, {}, both={"pw_fanout_kernel<%s, true, true, false>" % TNAME[dt]: 1},
                                never=("pw_fanout_slabs_kernel",)))
            else:   # the forward of an expand, the input gradient of a project
                out.append(swap("pwconv", (case, dt), {"pw_fanout_kernel<%s, true, true, false>" % TNAME[dt]: 1},
                                {"pw_fanout_slabs_kernel": 1}))
    return out


def _fanin_checks():
    # every case has one fan-in launch (K > 64): the input gradient of an expand, the forward of a project
    return [swap("pwconv", (case, dt), {"pw_fanin_pipe_kernel<%s, false, false, false>" % TNAME[dt]: 1},
                 {"pw_fanin_pipe_kernel<%s, false, true, false>" % TNAME[dt]: 1}) for dt in (BF16, F16) for case in PW_SWITCH_CASES]


def _dw_wgrad_checks():
    return [chk("dwconv", (shape, k, dt), child_never=("dw_wgrad_mfma_kernel",), ctrl_must={"dw_wgrad_mfma_kernel": 1})
            for dt in (BF16, F16) for k in (3, 5, 7) for shape in ((2, 4, 16, 32), (1, 3, 32, 64))]


def _onepass_checks():
    pair = {"bn_bwd_reduce_kernel": 1, "bn_bwd_apply_kernel": 1}
    out = []
    for dt in (BF16, F16):
        for training in (True, False):
            # (1, 2, 256, 256): N * HW / 8 is exactly BN1P_THREADS * BN1P_MAXCH = 8192 chunks, every thread holds 8
            for shape in ((2, 64, 8, 8), (3, 5, 4, 6), (1, 2, 256, 256)):
                out.append(swap("bn_bwd", (dt, training, shape), {"bn_bwd_onepass_kernel": 1}, pair))
            # 8193 chunks: one more than a workgroup holds -- the reduce / apply pair on both sides
            out.append(swap("bn_bwd", (dt, training, (1, 2, 24, 2731)), {}, {}, both=pair, never=("bn_bwd_onepass_kernel",)))
    return out


THIN = ("ct_out_kernel", "ct_in_kernel", "ct_wg_kernel")


def _conv_thin_checks():
    import test_hip_conv2d as tc
    cases = [c for c in tc.CASES if 3 in (c[1], c[2])]
    assert len(cases) == 4 and any(c[5] == 3 and c[2] == 3 for c in cases), cases   # stem and head, k = 5 and k = 3
    out = [chk("conv32", (c,), {"conv_f32_kernel": 2, "conv_f32_wgrad_kernel": 1}, THIN, {"|".join(THIN): None}) for c in cases]
    out += [chk("conv16", (c, BF16), {"conv_igemm_kernel": 2, "conv_wgrad_kernel": None}, THIN, {"|".join(THIN): None}) for c in cases]
    return out


def _pw_blocks_checks(extra):
    import test_hip_pw_wgrad_stream as ws
    out = []
    for s in ws.SHAPES:
        for role in ws.ROLES:
            for dt in (BF16, F16):
                out.append(chk("pw_wgrad", (s, role, dt, 0), {"pw_wgrad_direct_kernel<%s, 0>" % TNAME[dt]: 1}))
                out.append(chk("pw_wgrad_xf", (s, role, dt), {"pw_wgrad_direct_kernel": 1}))
    # SHAPES plan at most 64 splits, below either block count: one more shape at which this row's count changes the plan
    out.append(chk("pw_wgrad", (extra, "expand", BF16, 0), {"pw_wgrad_direct_kernel<%s, 0>" % TNAME[BF16]: 1}))
    return out


def _conv_blocks_checks():
    import test_hip_conv2d as tc
    return [chk("conv32", (c,)) for c in tc.F32_CASES]


BLOCK_CASES = [(2, 32, 32, 4, 7, True, BF16),    # mid 256: two slabs
               (2, 32, 32, 3, 3, True, BF16),    # mid 192: the generic fan-out kernel, the vector depthwise kernel
               (2, 32, 32, 6, 5, True, F16)]     # mid 384: three slabs


def _block_checks(profile, alt, dflt, bstat=False, skip_names=lambda case: False):
    """check_block on BLOCK_CASES under `profile`; alt / dflt: kernel names ({T}: element type, {K}: filter size) that the
    switched / default side runs and the other side does not.  check_block itself asserts the whole routing of its side"""
    import test_hip_composite16 as tb
    out = []
    for case in BLOCK_CASES:
        fmt = lambda names: {} if skip_names(case) else {n.format(T=TNAME[case[6]], K=case[4]): None for n in names}
        out.append(swap("block", (case, bool(bstat and tb.bstat_applies(case)), profile), fmt(alt), fmt(dflt)))
    return out


WG3, WG0 = "pw_wgrad_direct_kernel<{T}, 3>", "pw_wgrad_direct_kernel<{T}, 0>"
DWG_STORED, DWG_BX = "dw_wgrad_mfma_kernel<{T}, {K}, 1, true, false>", "dw_wgrad_mfma_kernel<{T}, {K}, 1, true, true>"
FANIN_FOLDED = "pw_fanin_pipe_kernel<{T}, false, true, true>"


def _rows():
    def row(id_, env, checks, probe=None):
        return dict(id=id_, env=dict(env), checks=checks, probe=probe)

    return [
        row("pw_wgrad_f32_direct", {"OFASR_PW_WGRAD_F32_DIRECT": "1"}, _f32_direct_checks),
        row("pw_fanout_slabs_0", {"OFASR_PW_FANOUT_SLABS": "0"}, lambda: _fanout_checks() + _block_checks(
            dict(fanout_slabs=False), ["pw_fanout_kernel<{T}, true, true, false>"], ["pw_fanout_slabs_kernel"],
            skip_names=lambda case: case[3] == 3)),
        row("pw_fanin_fast_0", {"OFASR_PW_FANIN_FAST": "0"}, lambda: _fanin_checks() + _block_checks(
            dict(fanin_fast=False), ["pw_fanin_pipe_kernel<{T}, true, false, false>", "pw_fanin_pipe_kernel<{T}, false, false, false>",
                                     "bn_bwd_apply_kernel<{T}, true, 1, false>"],
            ["pw_fanin_pipe_kernel<{T}, true, true, false>", FANIN_FOLDED])),
        row("dw_wgrad_mfma_0", {"OFASR_DW_WGRAD_MFMA": "0"}, lambda: _dw_wgrad_checks() + _block_checks(
            dict(dw_wgrad_mfma=False), ["dw_wgrad_vec_kernel"], ["dw_wgrad_mfma_kernel"])),
        row("bn_bwd_onepass_1", {"OFASR_BN_BWD_ONEPASS": "1"}, lambda: _onepass_checks() + _block_checks(
            dict(bn_onepass=True), ["bn_bwd_onepass_kernel"], ["bn_bwd_apply_kernel"])),
        row("conv_thin_0", {"OFASR_CONV_THIN": "0"}, _conv_thin_checks),
        row("pw_wgrad_blocks_96", {"OFASR_PW_WGRAD_BLOCKS": "96"}, lambda: _pw_blocks_checks((8, 64, 384, 4096)), "pw_wgrad_ws"),
        row("pw_wgrad_blocks_1024", {"OFASR_PW_WGRAD_BLOCKS": "1024"}, lambda: _pw_blocks_checks((17, 64, 384, 4096)), "pw_wgrad_ws"),
        row("conv_f32_wg_blocks_96", {"OFASR_CONV_F32_WG_BLOCKS": "96"}, _conv_blocks_checks, "conv_f32_wg_ws"),
        row("mbconv_wg1_bx_1", {"OFASR_MBCONV_WG1_BX": "1"}, lambda: _block_checks(dict(wg1_bx=True), [WG3], [WG0])),
        row("dw_wgrad_bx_0", {"OFASR_DW_WGRAD_BX": "0"}, lambda: _block_checks(dict(dw_wgrad_bx=False), [DWG_STORED], [DWG_BX])),
        row("mbconv_bn_bwd_fold_0", {"OFASR_MBCONV_BN_BWD_FOLD": "0"}, lambda: _block_checks(
            dict(bn_fold=False), ["bn_bwd_apply_kernel<{T}, true, 1, false>"], [FANIN_FOLDED])),
        row("mbconv_bn_coef_fold_0", {"OFASR_MBCONV_BN_COEF_FOLD": "0"}, lambda: _block_checks(
            dict(coef_fold=False), ["bn_bwd_coef_kernel"], [])),
        row("pw_epilogue_stats_0", {"OFASR_PW_EPILOGUE_STATS": "0"}, lambda: _block_checks(
            dict(epilogue_stats=False), ["bn_stats_kernel", "bn_finalize_kernel"], [])),
        # combinations whose scratch aliasing differs from both single settings (csrc/mbconv.hip: tA / tB / tC)
        row("wg1_bx_1+dw_wgrad_bx_0", {"OFASR_MBCONV_WG1_BX": "1", "OFASR_DW_WGRAD_BX": "0"}, lambda: _block_checks(
            dict(wg1_bx=True, dw_wgrad_bx=False), [WG3, DWG_STORED], [WG0, DWG_BX])),
        row("wg1_bx_1+bn_coef_fold_0", {"OFASR_MBCONV_WG1_BX": "1", "OFASR_MBCONV_BN_COEF_FOLD": "0"}, lambda: _block_checks(
            dict(wg1_bx=True, coef_fold=False), [WG3, "bn_bwd_coef_kernel"], [WG0])),
        row("wg1_bx_1+bn_bwd_stat", {"OFASR_MBCONV_WG1_BX": "1"}, lambda: _block_checks(dict(wg1_bx=True), [WG3], [WG0], bstat=True)),
        row("mbstack_kt_batch_0", {"OFASR_MBSTACK_KT_BATCH": "0"}, lambda: [
            chk("stack", (dt,), {"kt_fwd_kernel": None}, ("kt_fwd_batch_kernel",), {"kt_fwd_batch_kernel": None}) for dt in (BF16, None)]),
    ]


SWITCHES = _rows()
ROW = {r["id"]: r for r in SWITCHES}


# ---------------------------------------------------------------------------------------------------- running a check
def _count(table, part):
    """launches of the kernels whose name holds `part` (a|b: either)"""
    return sum(n for name, n in table.items() if any(p in name for p in part.split("|")))


def _table_of(ctx, c):
    ctx.C.reset_launch_counts()
    table = BODIES[c["body"]](ctx, *c["args"])
    return ctx.C.launch_table() if table is None else table


def _expect(c, side, table):
    must, never = c[side + "_must"], c[side + "_never"]
    names = sorted(set(must) | set(never) | set(c["child_must"]) | set(c["ctrl_must"]))
    print("  %s %s%r: %s" % (side, c["body"], c["args"], ", ".join("%s x%d" % (n, _count(table, n)) for n in names) or "-"))
    for part, n in must.items():
        got = _count(table, part)
        assert (got >= 1) if n is None else (got == n), "%s %s%r: %s ran %d time(s), expected %s\n%s" % (
            side, c["body"], c["args"], part, got, "at least once" if n is None else n, table)
    for part in never:
        assert _count(table, part) == 0, "%s %s%r: %s ran %d time(s), expected none\n%s" % (
            side, c["body"], c["args"], part, _count(table, part), table)


_CONTROL = {}    # (body, args) -> launch table: the control of a check runs once per session, whatever rows share it
_STATE = {"ctx": None, "dead": None, "probes": {}}


def _control(row):
    """the row's checks that expect something of the default side, in this process (the default environment)"""
    if _STATE["ctx"] is None:
        _STATE["ctx"] = Ctx(False)
    ctx = _STATE["ctx"]
    for name in row["env"]:
        assert name not in os.environ, "%s is set in the parent: the control must run under the default environment" % name
    for c in row["checks"]():
        key = (c["body"], repr(c["args"][:-1] if c["body"] == "block" else c["args"]))
        if c["ctrl_must"] or c["ctrl_never"]:
            if key not in _CONTROL:
                _CONTROL[key] = _table_of(ctx, c)
            _expect(c, "ctrl", _CONTROL[key])
    if row["probe"]:
        if row["probe"] not in _STATE["probes"]:
            _STATE["probes"][row["probe"]] = PROBES[row["probe"]](ctx)
        return _STATE["probes"][row["probe"]]
    return None


@pytest.mark.parametrize("row", SWITCHES, ids=[r["id"] for r in SWITCHES])
def test_switch_row(row):
    if _STATE["dead"]:
        pytest.fail("not started: an earlier child faulted or hung (%s)" % _STATE["dead"])
    probe = _control(row)
    torch.cuda.synchronize()
    env = dict(os.environ, **row["env"])
    t0 = time.time()
    try:
        out = subprocess.run([sys.executable, HERE, row["id"], json.dumps(probe)], env=env, cwd=os.path.dirname(HERE),
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _STATE["dead"] = "%s ran into its %d s limit" % (row["id"], CHILD_TIMEOUT)
        tail = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail("%s\n%s" % (_STATE["dead"], tail[-4000:]))
    print("row %s: child took %.1f s, status %d\n%s" % (row["id"], time.time() - t0, out.returncode, out.stdout[-6000:]))
    if out.returncode < 0 or out.returncode in FAULT_STATUS:
        _STATE["dead"] = "%s ended with status %d" % (row["id"], out.returncode)
    assert out.returncode == 0, "child of row %s ended with status %d:\n%s" % (row["id"], out.returncode, out.stdout[-4000:])


def _child(row_id, control_probe):
    row = ROW[row_id]
    for k, v in row["env"].items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    ctx = Ctx(True)
    if row["probe"]:
        mine = PROBES[row["probe"]](ctx)
        print("  probe %s: %s here, %s under the default environment" % (row["probe"], mine, control_probe))
        assert mine != control_probe, "%s changed nothing: the library ignored the switch" % (row["env"],)
    for c in row["checks"]():
        _expect(c, "child", _table_of(ctx, c))
    torch.cuda.synchronize()
    print("row %s: every check passed" % row_id)


if __name__ == "__main__":
    _child(sys.argv[1], json.loads(sys.argv[2]) if len(sys.argv) > 2 else None)
