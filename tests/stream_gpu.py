"""What the side-stream tests share (tests/test_streams_gpu.py; the table and the bars: tests/stream_cases.py): the delay, the side stream, and
the one procedure of every case.

    want    the call on the default stream with the right inputs (the route the rest of the suite holds to the oracle and the twins);
    decoy   the same call on a second valid input set of the same shapes; its outputs, and every caller-owned scratch as it left it, are kept
            and must differ from `want` beyond the case's bar in a tenth of the elements -- else the case could not fail;
    then, on a non-blocking side stream s: a delay, the right inputs copied over the decoy in place, the decoy's outputs and scratch copied
    over the buffers the entry writes once more (a clear or a memset that ran early is undone by it), the entry, a clone of its outputs.
    The entry has returned while the delay still runs (Event.query() is False: it did not synchronise, and everything it enqueued lies in the
    delay's shadow); s.synchronize() and nothing wider, and the clone is `want` under the case's bar.

Whatever the entry puts on another stream without a dependency on s reads the decoy, or has its clear undone.  Every buffer holds at every
moment bytes that a valid call left there -- no poison, no guard bands: a misplaced launch gives wrong values and cannot give a fault."""
import time

import torch

import stream_cases as sc

DELAY_MS = 50.0          # what a case's delay is sized to; the cap of any case's is CAP_MS
CAP_MS = 200.0
ENQUEUED = {}            # case -> (host milliseconds from the delay's launch to the entry's return, the delay's own milliseconds on the device)

_cycles_per_ms = None
_drawn = []              # every stream drawn stays alive: the pool then hands out another one next


def _timed(cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(int(cycles))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def cycles_per_ms():
    """torch.cuda._sleep's cycles in a millisecond, measured once per process."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        _timed(1000)                                   # (loads the kernel)
        cycles = 1 << 18
        while _timed(cycles) < 5.0:
            cycles *= 2
        _cycles_per_ms = cycles / min(_timed(cycles) for _ in range(3))
    return _cycles_per_ms


def delay(ms=DELAY_MS):
    """Keeps the current stream busy for `ms` milliseconds (torch.cuda._sleep, its cycles calibrated once per process by event timing: the
    shortest of three runs of a probe of 5 ms or more; measured, a delay of 50 ms takes 49.8 to 50.2) -> the event recorded behind it."""
    assert ms <= CAP_MS
    torch.cuda._sleep(int(ms * cycles_per_ms()))
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    return end


def handles_in_use(state=None):
    """The stream handles a side stream must differ from: 0, every lane stream of the process and the state's copy stream."""
    from ken_burns_effect_amd import _native
    taken = {0, torch.cuda.default_stream().cuda_stream}
    for streams in _native._LANE_STREAMS.values():
        taken |= {s.cuda_stream for s in streams}
    if state is not None:
        taken |= {s.cuda_stream for s in [state.get('copy_stream')] + list(state.get('lane_streams', [])) if s is not None}
    return taken


def side_stream(state=None):
    """A non-blocking stream (torch.cuda.Stream() creates its pool's with hipStreamNonBlocking: the null stream does not wait for it) whose
    handle is none of handles_in_use: torch hands out pooled streams and lane_streams_of draws from the same pool, so draw again until it differs."""
    taken = handles_in_use(state)
    for s in _drawn:
        if s.cuda_stream not in taken:
            return s
    for _ in range(64):
        _drawn.append(torch.cuda.Stream())
        if _drawn[-1].cuda_stream not in taken:
            break
    s = _drawn[-1]
    assert s.cuda_stream not in taken and s.cuda_stream != 0, 'no stream of the pool beside the lanes\' and the copy stream'
    return s


def tensors_of(result):
    return [t for t in (result if isinstance(result, (tuple, list)) else (result,)) if t is not None]


def arrays_of(tensors):
    return [t.detach().cpu().numpy().copy() for t in tensors]


def behind_delay(inputs, right, outputs, stale, call, state=None, asynchronous=True, what=''):
    """On a side stream, in this order: a delay; right[i] copied into inputs[i]; stale[i] copied into outputs[i]; call() under
    torch.cuda.stream(s); a clone of every device tensor it returns (host tensors are kept as they are: pinned buffers the stream fills).
    Asserts that the delay was still running when call() had returned (`asynchronous`), synchronises s alone -> the clones."""
    s = side_stream(state)
    cycles_per_ms()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        begin = torch.cuda.Event(enable_timing=True)
        begin.record()
        t0 = time.perf_counter()
        end = delay()
        for dst, src in zip(inputs, right):
            dst.copy_(src, non_blocking=True)
        for dst, src in zip(outputs, stale):
            dst.copy_(src, non_blocking=True)
        kept = [t.clone() if t.is_cuda else t for t in tensors_of(call())]
        running = not end.query()
        host_ms = (time.perf_counter() - t0) * 1e3
    if asynchronous:
        assert running, '%s: the delay had run out (or the entry synchronised) when the entry returned, %.2f ms after the delay\'s launch' % (what, host_ms)
    s.synchronize()
    took = begin.elapsed_time(end)
    if asynchronous:
        ENQUEUED[what] = (host_ms, took)
    print('%s: %s %.3f ms after the delay\'s launch; the delay took %.1f ms' % (what, 'enqueued' if asynchronous else 'returned (it synchronises)', host_ms, took))
    assert took <= CAP_MS, '%s: a delay of %.1f ms' % (what, took)
    return kept


def load(buffers, values):
    for dst, src in zip(buffers, values):
        dst.copy_(src)
    torch.cuda.synchronize()


def hold(what, bar, inputs, right, decoy, call, written=lambda: [], dirty=None, asynchronous=True, state=None, differ_in=None, view=lambda arrays: arrays):
    """The procedure of the module's docstring for one case.  inputs: the device tensors the entry reads, refilled in place; right, decoy: their
    two sets of values; call(): the entry -> its output tensors; written(): the caller-owned buffers the entry writes besides -- scratch, and
    outputs that are not fresh allocations -- as they exist after the first call; dirty(): a valid call more behind the decoy's, for entries
    whose result does not depend on their inputs (a clear: what it has to clear).  differ_in: the results the decoy must differ in (default: all); view(arrays): what of the results is compared (the units' bytes up to their end).
    -> (got, want) as lists of arrays, already compared."""
    def on_the_default_stream():
        result = tensors_of(call())
        torch.cuda.synchronize()                       # (a pinned buffer among the results is read below)
        return arrays_of(result)
    load(inputs, right)
    want = on_the_default_stream()
    load(inputs, decoy)
    other = on_the_default_stream()
    if dirty is not None:
        dirty()
    torch.cuda.synchronize()
    outputs = list(written())
    stale = [t.clone() for t in outputs]
    shares = sc.differing(view(other), view(want), bar)
    print('%s: the decoy differs beyond the bar in %s of its results\' elements' % (what, ', '.join('%.3f' % v for v in shares)))
    for i in (range(len(shares)) if differ_in is None else differ_in):
        assert shares[i] >= 0.1, '%s: the decoy\'s result %d differs from the right one in %.3f of its elements: the case could not fail' % (what, i, shares[i])
    got = arrays_of(behind_delay(inputs, right, outputs, stale, call, state=state, asynchronous=asynchronous, what=what))
    sc.check(view(got), view(want), bar, what)
    return got, want
