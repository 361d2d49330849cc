"""Exponential moving average (EMA) of the weights during training.

The definition, in numpy (the host statement the kernel of csrc/ema.hip is pinned to, bit for bit): the shadow `e` holds
one fp32 value per element of every tensor of network.parameters().  After optimizer step number t (t = 0 for the first
step of the run, continued across a resume), with parameters p:

    d_t = min(D, (1 + t) / (10 + t))       decay_at: D = --ema-decay, the warm-up of TF / timm, in Python floats
    w   = float32(1 - d_t)
    e'  = e + float32(w * float32(p - e))  update_np: three fp32 operations, each rounded once, no fma

`plan_chunks` states how a list of tensor sizes becomes the rows of the kernel's table; `ParamEMA` owns the shadow (one
flat fp32 GPU buffer) and the table and runs update / swap as ONE launch each, whatever the number of tensors
(ops.ema_update / ops.ema_swap).  `averaged_state_dict` is what the checkpoint readers load under --ema.

Buffers are not averaged: BatchNorm running statistics stay the network's own (search and export re-estimate them, the
fixed-architecture loop keeps them frozen).
"""
import numpy as np
import torch


def check_decay(decay, what="ema_decay"):
    """0 <= decay < 1 as a float, or a ValueError that names `what`"""
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number in [0, 1), got %r" % (what, decay))
    if not (0.0 <= d < 1.0):          # refuses nan too
        raise ValueError("%s must lie in [0, 1), got %r" % (what, decay))
    return d


def decay_at(t, decay):
    """the decay of update number t (the first is t = 0): min(D, (1 + t) / (10 + t))"""
    return min(float(decay), (1.0 + t) / (10.0 + t))


def weight_at(t, decay):
    """w of update number t as the fp32 value the kernel is given"""
    return np.float32(1.0 - decay_at(t, decay))


def update_np(e, p, w):
    """e + float32(w * float32(p - e)) over fp32 arrays: three fp32 operations, each rounded once"""
    e = np.asarray(e, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    w = np.float32(w)
    d = np.subtract(p, e, dtype=np.float32)
    m = np.multiply(w, d, dtype=np.float32)
    return np.add(e, m, dtype=np.float32)


def plan_chunks(sizes, chunk):
    """[(tensor index, first element, count)]: each tensor cut from its own first element into pieces of at most `chunk`
    elements, in order; a zero-size tensor gives no row; a row never spans two tensors"""
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError("chunk must be positive, got %r" % (chunk,))
    rows = []
    for i, n in enumerate(sizes):
        n = int(n)
        if n < 0:
            raise ValueError("tensor %d has negative size %d" % (i, n))
        for off in range(0, n, chunk):
            rows.append((i, off, min(chunk, n - off)))
    return rows


def averaged_state_dict(checkpoint, fname=None):
    """checkpoint["state_dict"] with the tensors of checkpoint["ema"]["state_dict"] laid over it: the averaged parameters
    and the network's own buffers.  A checkpoint without an "ema" entry (a run without --ema-decay) is refused."""
    where = "checkpoint" if fname is None else "checkpoint %s" % fname
    ema = checkpoint.get("ema") if isinstance(checkpoint, dict) else None
    if not isinstance(ema, dict) or "state_dict" not in ema:
        raise ValueError("%s has no \"ema\" entry: it was not written by a run with --ema-decay, so there are no "
                         "averaged weights to load" % where)
    if "state_dict" not in checkpoint:
        raise ValueError("%s has no \"state_dict\" entry" % where)
    out = dict(checkpoint["state_dict"])
    for name, t in ema["state_dict"].items():
        if name not in out:
            raise ValueError("%s: averaged tensor %r has no counterpart in \"state_dict\"" % (where, name))
        if tuple(out[name].shape) != tuple(t.shape):
            raise ValueError("%s: averaged tensor %r has shape %s, \"state_dict\" has %s" % (
                where, name, tuple(t.shape), tuple(out[name].shape)))
        out[name] = t
    return out


class ParamEMA(object):
    """The shadow of `params` (an iterable of (name, parameter), e.g. network.named_parameters()) and its kernel table.

    The shadow is one flat fp32 GPU buffer with one view per parameter (each view starts on a 16-byte boundary, so a
    row takes the kernel's vector path whenever the parameter's own storage does).  The device table is built once from
    plan_chunks and rebuilt when the tuple of parameter data_ptr()s changes (a .to() does that, load_state_dict does
    not).  `updates` -- the t of the next update -- lives on the host."""

    def __init__(self, params, decay):
        from . import ops
        self._ops = ops
        self.decay = check_decay(decay, "decay")
        named = list(params)
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        if len(set(self.names)) != len(self.names):
            raise ValueError("parameter names are not unique")
        for n, p in named:
            if not p.is_cuda:
                raise ValueError("parameter %s is on %s: the weight average runs on the GPU (no CPU fallback)" % (n, p.device))
            if p.dtype != torch.float32:
                raise ValueError("parameter %s is %s: master weights are fp32" % (n, p.dtype))
            if not p.is_contiguous():
                raise ValueError("parameter %s is not contiguous" % n)
        if self.params and len({p.device for p in self.params}) != 1:
            raise ValueError("parameters live on more than one device")
        self.device = self.params[0].device if self.params else torch.device("cuda")
        self.chunk = int(ops.ema_chunk())
        self.sizes = [p.numel() for p in self.params]
        self.elements = sum(self.sizes)
        offs, total = [], 0
        for n in self.sizes:
            offs.append(total)
            total += (n + 3) // 4 * 4
        self.flat = torch.zeros(max(total, 4), dtype=torch.float32, device=self.device)
        self.views = [self.flat[o:o + n].view(p.shape) for o, n, p in zip(offs, self.sizes, self.params)]
        self._plan = plan_chunks(self.sizes, self.chunk)
        self.rows = len(self._plan)
        self._ptrs, self.table = None, None
        self._swapped = False
        self.updates = 0
        self.reset()

    # ----------------------------------------------------------------------------------------------- table
    def _table(self):
        ptrs = tuple(p.data_ptr() for p in self.params)
        if ptrs != self._ptrs:
            host = np.empty((self.rows, 3), dtype=np.int64)
            shadow = [v.data_ptr() for v in self.views]
            for r, (i, off, cnt) in enumerate(self._plan):
                host[r, 0], host[r, 1], host[r, 2] = ptrs[i] + 4 * off, shadow[i] + 4 * off, cnt
            self.table = torch.from_numpy(host).to(self.device) if self.rows else \
                torch.zeros((0, 3), dtype=torch.int64, device=self.device)
            self._ptrs = ptrs
        return self.table

    # --------------------------------------------------------------------------------------------- kernels
    def reset(self):
        """the shadow becomes a copy of the parameters as they are now, updates = 0"""
        if self._swapped:
            raise RuntimeError("the parameters hold the averaged weights (inside swap()): swap back first")
        with torch.no_grad():
            if self.params:
                torch._foreach_copy_(self.views, [p.detach() for p in self.params])
        self.updates = 0

    def update(self):
        """update number `updates`: one launch on the current stream, no host read, no allocation"""
        if self._swapped:
            raise RuntimeError("the parameters hold the averaged weights (inside swap()): swap back first")
        self._ops.ema_update(self._table(), self.rows, weight_at(self.updates, self.decay), elements=self.elements)
        self.updates += 1

    def swap(self):
        """exchange parameters and shadow (one launch), then ops.clear_infer_cache(): the kernel writes the parameters
        behind their version counters, and the inference operand cache and GraphedEval recognise weights by (address,
        version) -- without the clear a validation would replay the operands of the weights that were there before"""
        self._ops.ema_swap(self._table(), self.rows, elements=self.elements)
        self._swapped = not self._swapped
        self._ops.clear_infer_cache()

    # ------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """{"decay", "updates", "state_dict": {parameter name: CPU fp32 tensor}} -- tensors, floats, ints and strings
        only.  The averaged values, on either side of a swap()."""
        src = self.params if self._swapped else self.views
        return {"decay": float(self.decay), "updates": int(self.updates),
                "state_dict": {n: t.detach().to("cpu", copy=True).contiguous() for n, t in zip(self.names, src)}}

    def load_state_dict(self, d):
        """values and `updates` of a state_dict(); a name or shape that does not match is refused, by name"""
        if self._swapped:
            raise RuntimeError("the parameters hold the averaged weights (inside swap()): swap back first")
        sd = d["state_dict"]
        missing = [n for n in self.names if n not in sd]
        extra = [n for n in sd if n not in set(self.names)]
        if missing or extra:
            raise ValueError("averaged weights do not match the network: missing %s, unexpected %s" % (missing, extra))
        for n, v in zip(self.names, self.views):
            if tuple(sd[n].shape) != tuple(v.shape):
                raise ValueError("averaged tensor %s has shape %s, the parameter has %s" % (
                    n, tuple(sd[n].shape), tuple(v.shape)))
            if sd[n].dtype != torch.float32:
                raise ValueError("averaged tensor %s is %s, not fp32" % (n, sd[n].dtype))
        with torch.no_grad():
            for n, v in zip(self.names, self.views):
                v.copy_(sd[n])
        self.updates = int(d["updates"])
