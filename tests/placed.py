"""Operand placement with guard bands, for tests that hand a kernel pointers which are NOT what the allocator returns.

One buffer per operand, laid out as

    [ front guard | lead | payload | back guard ]

The buffer base is 16-byte aligned, so the payload's address is `lead_bytes` mod 16.  Both guards are at least 4096
bytes and at least two H*W planes of the tensor, so an access that is one plane off still lands inside the buffer:
an overrun fails an assertion and never touches memory the test does not own.  Nothing here places a tensor at the
end of an allocation.

    role "in"   guards (and the lead) hold 0xFF bytes -- NaN in f32, f16, bf16 and f64, so a load before x[0] or past
                x[-1] poisons the result -- and check() also demands that the payload still equals `t` byte for byte.
    role "out"  guards hold 0xA5 bytes; the payload is pre-filled with 0xFF bytes (NaN), so an element the kernel never
                wrote shows up in the comparison with the reference.

check() runs after torch.cuda.synchronize() and reports the byte offset of the first damaged byte relative to the payload
(negative: before it; >= nbytes: past it).

Placements by lead:
    P0  lead 0                     aligned base: the vector kernels run and the guards check their edges
    P1  one element (2 / 4 bytes)  no vector access is legal
    P8  8 bytes                    fit for 8-byte vectors, not for 16-byte ones
"""
import torch

GUARD_MIN = 4096
IN_FILL = 0xFF      # NaN in every float type the kernels take; plain 0xFF for integer types
OUT_GUARD = 0xA5
OUT_FILL = 0xFF     # the canary an output payload starts with


class GuardError(AssertionError):
    pass


def lead_of(name, elem_size):
    """lead bytes of the placement `name` ("P0" / "P1" / "P8") for elements of `elem_size` bytes"""
    return {"P0": 0, "P1": int(elem_size), "P8": 8}[name]


def _plane_bytes(t):
    if t.dim() >= 4:
        n = int(t.shape[-1]) * int(t.shape[-2])
    elif t.dim() >= 1:
        n = int(t.shape[-1])
    else:
        n = 1
    return n * t.element_size()


def _round16(n):
    return (int(n) + 15) // 16 * 16


class Placement(object):
    """bookkeeping of one placed operand; `t` is the payload view, `ptr` its address"""

    def __init__(self, buf, lo, nbytes, role, lead, name, guard_fill, orig):
        self.buf, self.lo, self.nbytes, self.role, self.lead, self.name = buf, lo, nbytes, role, lead, name
        self.guard_fill, self.orig = guard_fill, orig
        self.t = None

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def __repr__(self):
        shape = tuple(self.t.shape) if self.t is not None else (self.nbytes,)
        dt = str(self.t.dtype).replace("torch.", "") if self.t is not None else "bytes"
        return "<%s %s %s%s lead=%d (address %% 16 = %d)>" % (self.name or "operand", self.role, dt, list(shape), self.lead,
                                                             self.ptr % 16)

    def payload_bytes(self):
        return self.buf[self.lo:self.lo + self.nbytes]

    def unwritten(self):
        """bool tensor, shaped like the payload: elements that still hold the 0xFF canary in every byte"""
        es = self.t.element_size()
        return (self.payload_bytes().view(-1, es) == OUT_FILL).all(dim=1).view(self.t.shape)


def place(t, lead_bytes, role, name=""):
    """a contiguous view, at `lead_bytes` mod 16, of a guard-banded copy of `t` (role "in") or of a canary-filled payload
    of t's shape and dtype (role "out").  The view carries its bookkeeping as `.placement`."""
    assert role in ("in", "out"), role
    es = t.element_size()
    lead = int(lead_bytes)
    assert 0 <= lead < 16 and lead % es == 0, "lead %d is not a whole number of %d-byte elements below 16" % (lead, es)
    nbytes = t.numel() * es
    guard = _round16(max(GUARD_MIN, 2 * _plane_bytes(t)))
    total = guard + 16 + _round16(nbytes) + guard
    fill = IN_FILL if role == "in" else OUT_GUARD
    buf = torch.full((total,), fill, dtype=torch.uint8, device=t.device)
    assert buf.data_ptr() % 16 == 0, "buffer base is not 16-byte aligned"
    lo = guard + lead
    orig = None
    if role == "in":
        orig = t.detach().contiguous().reshape(-1).view(torch.uint8).clone()
        buf[lo:lo + nbytes] = orig
    else:
        buf[lo:lo + nbytes] = OUT_FILL
    p = Placement(buf, lo, nbytes, role, lead, name, fill, orig)
    v = buf[lo:lo + nbytes].view(t.dtype).view(t.shape)
    assert v.is_contiguous() and v.data_ptr() == p.ptr and v.data_ptr() % 16 == lead
    p.t = v
    v.placement = p
    return v


def workspace(nbytes, device="cpu", name="workspace"):
    """exactly `nbytes` of 16-byte aligned scratch pre-filled with 0xFF, 0xA5 guards on both sides.  Returns the
    Placement (`.ptr`, `.nbytes`; `.t` is the scratch as bytes)."""
    nbytes = int(nbytes)
    guard = GUARD_MIN
    buf = torch.full((guard + _round16(nbytes) + 16 + guard,), OUT_GUARD, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0, "buffer base is not 16-byte aligned"
    buf[guard:guard + nbytes] = OUT_FILL
    p = Placement(buf, guard, nbytes, "ws", 0, name, OUT_GUARD, None)
    p.t = buf[guard:guard + nbytes]
    assert p.ptr % 16 == 0
    return p


def _first_diff(got, want_fill=None, want=None):
    bad = (got != want_fill) if want is None else (got != want)
    n = int(bad.sum())
    if n == 0:
        return None
    return int(bad.nonzero()[0, 0]), n


def check(placed, payload=True):
    """guards byte-identical to what they were; for role "in" the payload too (payload=False: an operand the call both
    reads and updates, such as running statistics).  `placed` is what place() or workspace() returned.  Call after
    torch.cuda.synchronize()."""
    p = placed if isinstance(placed, Placement) else placed.placement
    hi = p.lo + p.nbytes
    d = _first_diff(p.buf[:p.lo], p.guard_fill)
    if d is not None:
        raise GuardError("%r: WRITE before the payload: %d byte(s) of the front guard changed, first at payload offset %d"
                         % (p, d[1], d[0] - p.lo))
    d = _first_diff(p.buf[hi:], p.guard_fill)
    if d is not None:
        raise GuardError("%r: WRITE past the payload: %d byte(s) of the back guard changed, first at payload offset %d "
                         "(%d past the end)" % (p, d[1], p.nbytes + d[0], d[0]))
    if p.role == "in" and payload:
        d = _first_diff(p.buf[p.lo:hi], want=p.orig)
        if d is not None:
            raise GuardError("%r: input modified: %d byte(s) changed, first at payload offset %d" % (p, d[1], d[0]))


def check_all(*placed):
    for p in placed:
        if p is not None:
            check(p)
