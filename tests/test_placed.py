"""The placement helper can fail: stand-in "kernels" written in torch, each with one of the faults the GPU placement
tests look for, must be caught by placed.check or by the comparison with the reference.  CPU tensors, no GPU."""
import numpy as np
import pytest
import torch

import placed
from placed import GuardError, check, place, workspace

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LEADS = ["P0", "P1", "P8"]


def _x(dtype, shape=(2, 3, 5, 7)):
    n = int(np.prod(shape))
    return (torch.arange(n, dtype=torch.float32).reshape(shape) / 8.0 - 3.0).to(dtype)


def _flat_around(p):
    """the whole buffer as elements of the payload's dtype, and the index of payload element 0 in it (the stand-ins
    reach outside the payload through this, as a kernel with a wrong index would)"""
    pl = p.placement
    es = p.element_size()
    start = pl.lo % es
    whole = pl.buf[start:start + (pl.buf.numel() - start) // es * es].view(p.dtype)
    return whole, (pl.lo - start) // es


@pytest.mark.parametrize("dtype", DTYPES + [torch.int8, torch.float64])
@pytest.mark.parametrize("lead", LEADS)
def test_layout(dtype, lead):
    t = _x(torch.float32).to(dtype)
    lb = placed.lead_of(lead, t.element_size())
    x = place(t, lb, "in", "x")
    assert x.is_contiguous() and x.dtype == dtype and x.shape == t.shape and torch.equal(x, t)
    assert x.data_ptr() % 16 == lb and x.placement.buf.data_ptr() % 16 == 0
    pl = x.placement
    plane = 5 * 7 * t.element_size()
    assert pl.lo - pl.lead >= max(4096, 2 * plane) and pl.buf.numel() - pl.lo - pl.nbytes >= max(4096, 2 * plane)
    check(x)
    y = place(t, lb, "out", "y")
    assert y.data_ptr() % 16 == lb and bool(y.placement.unwritten().all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(y).all())                       # the canary is NaN in every float type
        whole, i0 = _flat_around(x)
        assert bool(torch.isnan(whole[i0 - 1])) and bool(torch.isnan(whole[i0 + t.numel()]))   # and so are "in" guards
    assert "lead=%d" % lb in repr(pl) and "x" in repr(pl)


def test_guard_covers_two_planes_of_a_large_tensor():
    t = torch.zeros((1, 1, 64, 64), dtype=torch.float32)
    pl = place(t, 4, "in").placement
    assert pl.lo - pl.lead >= 2 * 64 * 64 * 4 and pl.buf.numel() - pl.lo - pl.nbytes >= 2 * 64 * 64 * 4


def _well_behaved(x, y):
    y.copy_(x * 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lead", LEADS)
def test_well_behaved_kernel_passes(dtype, lead):
    t = _x(dtype)
    lb = placed.lead_of(lead, t.element_size())
    x, y = place(t, lb, "in", "x"), place(t, lb, "out", "y")
    _well_behaved(x, y)
    check(x)
    check(y)
    assert torch.equal(y, t * 2) and not bool(y.placement.unwritten().any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lead", LEADS)
def test_write_one_element_before_is_caught(dtype, lead):
    t = _x(dtype)
    y = place(t, placed.lead_of(lead, t.element_size()), "out", "y")
    _well_behaved(t, y)
    whole, i0 = _flat_around(y)
    whole[i0 - 1] = 1.0
    with pytest.raises(GuardError, match=r"before the payload.*payload offset -%d" % t.element_size()):
        check(y)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lead", LEADS)
def test_write_one_element_after_is_caught(dtype, lead):
    t = _x(dtype)
    y = place(t, placed.lead_of(lead, t.element_size()), "out", "y")
    _well_behaved(t, y)
    whole, i0 = _flat_around(y)
    whole[i0 + t.numel()] = 1.0
    with pytest.raises(GuardError, match=r"past the payload.*payload offset %d \(0 past" % (t.numel() * t.element_size())):
        check(y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_element_is_caught(dtype):
    t = _x(dtype)
    y = place(t, t.element_size(), "out", "y")
    y.view(-1)[:-1].copy_((t * 2).view(-1)[:-1])          # the last element is never stored
    check(y)                                              # the guards are fine ...
    assert int(y.placement.unwritten().sum()) == 1        # ... the canary is still there
    with pytest.raises(AssertionError):                   # ... and it is a NaN for the comparison with the reference
        from conftest import assert_close
        assert_close(y.float().numpy(), (t * 2).float().numpy(), 1e-2, 1e-2, "y")


@pytest.mark.parametrize("dtype", DTYPES)
def test_modified_input_is_caught(dtype):
    t = _x(dtype)
    x = place(t, 8, "in", "x")
    x[1, 2, 3, 4] += 1.0
    off = ((1 * 3 + 2) * 5 + 3) * 7 + 4
    with pytest.raises(GuardError, match=r"input modified") as e:
        check(x)
    got = int(str(e.value).rsplit("payload offset ", 1)[1])    # the first changed byte lies inside that element
    assert off * t.element_size() <= got < (off + 1) * t.element_size()


@pytest.mark.parametrize("nbytes", [1, 100, 512, 4097])
def test_workspace_overrun_by_one_byte_is_caught(nbytes):
    ws = workspace(nbytes)
    assert ws.ptr % 16 == 0 and ws.t.numel() == nbytes and bool((ws.t == 0xFF).all())
    ws.t.fill_(3)                                         # using all of it is fine
    check(ws)
    ws.buf[ws.lo + nbytes] = 3                            # one byte past the queried size
    with pytest.raises(GuardError, match=r"past the payload.*\(0 past"):
        check(ws)
    ws2 = workspace(nbytes)
    ws2.buf[ws2.lo - 1] = 3
    with pytest.raises(GuardError, match=r"before the payload.*offset -1"):
        check(ws2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lead", LEADS)
def test_read_before_input_poisons_the_result(dtype, lead):
    """a stand-in that folds the element before x[0] (or after x[-1]) into its result reads a NaN from the guard, and
    the assertion on the result catches it; the guards themselves are intact (a read damages nothing)."""
    from conftest import assert_close
    t = _x(dtype)
    x = place(t, placed.lead_of(lead, t.element_size()), "in", "x")
    whole, i0 = _flat_around(x)
    n = t.numel()
    ref = (t.float().view(-1)[:-1] + t.float().view(-1)[1:]).numpy()
    good = (whole[i0:i0 + n - 1].float() + whole[i0 + 1:i0 + n].float()).numpy()
    assert_close(good, ref, 1e-6, 1e-6, "sum of neighbours")
    for s in (-1, 1):                                     # the same "kernel", its window one element off
        bad = (whole[i0 + s:i0 + s + n - 1].float() + whole[i0 + s + 1:i0 + s + n].float()).numpy()
        assert np.isnan(bad).sum() == 1
        with pytest.raises(AssertionError):
            assert_close(bad, ref, 1e-6, 1e-6, "sum of neighbours")
    check(x)
