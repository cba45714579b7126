"""Stream-order checks for the `_device` entry points (include/vecchio_amd.h: "enqueued on hip_stream without a host wait").  TESTS ONLY.

A value test on the NULL stream with a device synchronisation on either side cannot see an enqueue on the wrong stream, a missing fork or
join of an internal stream, scratch reused too early or a host struct captured by pointer.  ordered_call() makes each of them give wrong
VALUES, every time: the call is enqueued on a non-blocking stream S of the caller's own, behind a bounded delay, while its inputs still
hold POISON (valid input with another answer); the true inputs arrive on S behind the delay, the outputs (prefilled with a CANARY) are
copied out on S behind the call and refilled with the canary at once, and the host structs are overwritten as soon as the call returns.
Work that does not wait for S reads poison; work that S does not wait for leaves canary (or a torn image) in the copy.  The expected values
come from reference_call(): the same call with stream = NULL and a device synchronisation on either side, which the other GPU tests hold to
numpy and the oracle.  Nothing here faults, hangs or retries: every buffer is valid whatever the order, and the delay is a few tens of ms.
"""
import ctypes as C
import time

import numpy as np

DELAY_MS = 25.0          # of the delay in front of a call: long against the host time of an enqueue, nowhere near a hang
DELAY_MS_MAX = 50.0
CANARY_F32 = 7.0
CANARY_BYTE = 0xAA
_cal = {}


def _timed(stream, enqueue):
    """ms of what enqueue() puts on `stream`, by two events (waits: calibration only, never inside a check)"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        enqueue()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _calibrate():
    """once per session: how to make a delay — torch.cuda._sleep and its cycles per ms, or (a torch build without it) a fixed chain of
    large elementwise operations and its links per ms.  The unit is grown tenfold from a small one until it takes 2 ms, so that no
    calibration run is longer than a few tens of ms either."""
    import torch
    if _cal:
        return _cal
    s = torch.cuda.Stream()
    if hasattr(torch.cuda, "_sleep"):
        unit = lambda n: torch.cuda._sleep(int(n))
        kind, n = "torch.cuda._sleep", 100_000
    else:
        slab = torch.ones(1 << 24, dtype=torch.float32, device="cuda:0")

        def unit(n):
            for _ in range(int(n)):
                slab.mul_(1.0)
        kind, n = "elementwise chain", 4
    _timed(s, lambda: unit(n))                              # (the first launch loads the kernel)
    ms = _timed(s, lambda: unit(n))
    while ms < 2.0 and n < 10 ** 10:
        n *= 10
        ms = _timed(s, lambda: unit(n))
    _cal.update(kind=kind, unit=unit, per_ms=n / ms)
    return _cal


def enqueue_delay(stream, ms=DELAY_MS):
    """a delay of about `ms` on `stream`; returns the ms asked for"""
    import torch
    assert 0 < ms <= DELAY_MS_MAX
    cal = _calibrate()
    with torch.cuda.stream(stream):
        cal["unit"](max(1, cal["per_ms"] * ms))
    return ms


def measured_delay_ms(ms=DELAY_MS):
    """what a delay of `ms` really takes (two events on a stream of its own: for the report, not asserted)"""
    import torch
    cal = _calibrate()
    key = ("measured", ms)
    if key not in cal:
        s = torch.cuda.Stream()
        cal[key] = _timed(s, lambda: cal["unit"](max(1, cal["per_ms"] * ms)))
    return cal[key]


def canary_of(t):
    return CANARY_F32 if t.is_floating_point() else CANARY_BYTE


def fill(t, value):
    """every element of a float tensor, every BYTE of any other, := value"""
    import torch
    if t.is_floating_point():
        t.fill_(float(value))
    else:
        t.view(torch.uint8).fill_(int(value))


def put(x, v):
    """x := v, a tensor of x's shape or a fill value (see fill)"""
    import torch
    if isinstance(v, torch.Tensor):
        x.copy_(v, non_blocking=True)
    else:
        fill(x, v)


def overwrite(struct, other):
    """a host struct the library was handed := another valid one of its type"""
    assert type(struct) is type(other) and bytes(struct) != bytes(other)
    C.memmove(C.byref(struct), C.byref(other), C.sizeof(struct))


def clone(struct):
    return type(struct).from_buffer_copy(struct)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.itemsize == 1 else a.view(np.uint32)


def same(got, want):
    return all(g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want)) and len(got) == len(want)


def describe_difference(got, want, names=None):
    out = []
    for i, (g, w) in enumerate(zip(got, want)):
        bad = bits(g) != bits(w)
        if bad.any():
            canary = np.full(1, canary_of_numpy(g), g.dtype)
            is_canary = (bits(g) == bits(np.broadcast_to(canary, g.shape))) & bad
            out.append(f"{names[i] if names else i}: {int(bad.sum())} of {bad.size} words differ, {int(is_canary.sum())} of them hold the canary")
    return "; ".join(out) or "equal"


def canary_of_numpy(a):
    return CANARY_F32 if a.dtype.kind == "f" else np.frombuffer(bytes([CANARY_BYTE]) * a.dtype.itemsize, a.dtype)[0]


class Ctx:
    """what a call sees: the stream to enqueue on — `ptr` for the library (None: the NULL stream), `stream` for the copies that go
    between its stages — barrier() between two stages, and mark() where condition (a) is to be judged (default: when call returns)."""

    def __init__(self, stream, ptr, ordered, e_in=None):
        self.stream, self.ptr, self.ordered, self._e_in, self.pending = stream, ptr, ordered, e_in, None

    def barrier(self):
        """reference run: a device synchronisation; ordered run: nothing (the stream alone orders the stages)"""
        if not self.ordered:
            import torch
            torch.cuda.synchronize()

    def mark(self):
        """condition (a), judged once: the true inputs have not arrived yet, so the host has not waited for the stream"""
        if self.ordered and self.pending is None:
            self.pending = not self._e_in.query()

    def copy_out(self, dst, src):
        """dst := src behind the stage just enqueued, src := canary behind that"""
        import torch
        self.barrier()
        with torch.cuda.stream(self.stream):
            dst.copy_(src, non_blocking=True)
            fill(src, canary_of(src))
        self.barrier()


def reference_call(inputs, values, call, outputs):
    """The reference run: `values` (the true inputs, or the poison) in place, the outputs canary, a device synchronisation, the call on the
    NULL stream, a device synchronisation.  Returns (the outputs as numpy arrays, the call's wall ms between the two synchronisations)."""
    import torch
    in_ptrs = {x.data_ptr() for x in inputs}
    for o in outputs:
        if o.data_ptr() not in in_ptrs:
            fill(o, canary_of(o))
    for x, v in zip(inputs, values):
        put(x, v)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(Ctx(torch.cuda.default_stream(), None, False))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    got = [o.cpu().numpy().copy() for o in outputs]
    return got, ms


def ordered_call(S, inputs, poison, call, outputs, canary=None, true=None, delay_ms=DELAY_MS, library_stream=None):
    """One check (see the module's text).  inputs: device tensors the call reads (an in/out buffer is listed in outputs too); poison and
    true: per input a tensor or a fill value; outputs: device tensors the call writes, or snapshots that call() copies out behind its
    stages with ctx.copy_out(); canary: per output, default 7.0f / 0xAA bytes.  call(ctx) enqueues on ctx.ptr / ctx.stream and overwrites
    the host structs it passed as soon as each library call returns.  library_stream: the self-test's mis-ordered caller — the library
    call goes on THAT stream while everything else stays on S.
    Returns the outputs as numpy arrays after S.synchronize(); raises if condition (a) did not hold (inconclusive, never a pass)."""
    import torch
    assert S.cuda_stream != 0 and S != torch.cuda.default_stream() and S != torch.cuda.current_stream(), \
        "S must be a stream of the caller's own: neither the NULL stream nor the current one"
    assert len(inputs) == len(poison) == len(true)
    canary = list(canary) if canary is not None else [canary_of(o) for o in outputs]
    in_ptrs = {x.data_ptr() for x in inputs}
    staged = [t.clone() if isinstance(t, torch.Tensor) else t for t in true]       # (on the device before the check starts)
    for o, c in zip(outputs, canary):
        if o.data_ptr() not in in_ptrs:
            fill(o, c)
    for x, p in zip(inputs, poison):                                               # 1. poison in place
        put(x, p)
    results = [torch.empty_like(o) for o in outputs]
    torch.cuda.synchronize()
    # ---- from here to S.synchronize(): S only, no host wait, no NULL-stream work
    e_in = torch.cuda.Event()
    enqueue_delay(S, delay_ms)                                                     # 2.
    with torch.cuda.stream(S):                                                     # 3.
        for x, t in zip(inputs, staged):
            put(x, t)
        e_in.record(S)
    lib = library_stream if library_stream is not None else S
    ctx = Ctx(S, lib.cuda_stream, True, e_in)
    assert torch.cuda.current_stream() != S
    call(ctx)                                                                      # 4.
    ctx.mark()                                                                     # 5.
    with torch.cuda.stream(S):                                                     # 6.
        for r, o, c in zip(results, outputs, canary):
            r.copy_(o, non_blocking=True)
            fill(o, c)
    S.synchronize()                                                                # 7.
    if library_stream is not None:
        library_stream.synchronize()
    assert ctx.pending, ("INCONCLUSIVE: the true inputs had arrived when the call returned — the call waited on the host, or the delay "
                         f"({delay_ms} ms asked) is shorter than the enqueue")
    return [r.cpu().numpy() for r in results]


def concurrent_stream(S):
    """A second stream whose work really overtakes a delay on S (streams share a few hardware queues: one that shares S's queue would
    run behind S's delay by accident).  Probed with a 5 ms delay on S and an event on the candidate; None if none of four is free."""
    import torch
    for _ in range(4):
        s2 = torch.cuda.Stream()
        torch.cuda.synchronize()
        done_s, done_2 = torch.cuda.Event(), torch.cuda.Event()
        enqueue_delay(S, 5.0)
        done_s.record(S)
        with torch.cuda.stream(s2):
            torch.zeros(16, device="cuda:0").add_(1.0)
            done_2.record(s2)
        done_2.synchronize()
        overtook = not done_s.query()
        S.synchronize()
        if overtook:
            return s2
    return None
