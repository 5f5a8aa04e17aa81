"""The GPU harness of tests/test_gif_gpu.py: kbe_gif_encode called through gif.py's typed binding with sentinels around everything it may
write (tests/encoder_gpu.py does the same for the entries of kbe.h, through _native), and what the tests of the three entries share."""
import ctypes

import numpy as np
import torch

import gif_cases as gc
from guarded import GUARD, SENTINEL, Guard


def gif():
    from ken_burns_effect_amd import gif as module
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    module.load()
    return module


def stream():
    from ken_burns_effect_amd import _native
    return _native._stream()


def on_device(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.array(a)).cuda()           # (a copy: the cases' arrays are read-only)


def pointers_of(frames, n=None):
    count, H, Wt, _ = frames.shape
    n = count if n is None else n
    return (ctypes.c_void_p * max(n, 1))(*[frames.data_ptr() + i * H * Wt * 3 for i in range(n)])


def run(frames, lut, cap, flags=0, dither=0, delay_cs=4, W=None, H=None, stride=None, n=None, shift=0, status_before=7, change=None):
    """kbe_gif_encode on a uint8 device tensor [n,H,Wt,3] (W <= Wt: the rows' stride is Wt's) with a buffer of `cap` bytes (`shift` bytes off
    its allocation's start) followed by GUARD bytes, everything the call may write filled with sentinels first.  The scratch is exactly
    kbe_gif_scratch_bytes, rounded up only to the 8 bytes its alignment check asks for, every byte of it 0xFF, and like the offsets and the
    status word between two guard bands (tests/guarded.py).  change(args): the last word on the argument list -- a dict by the header's
    names.  -> (rc, offsets, status, the buffer with its guard, whether the scratch still holds its poison)."""
    G = gif()
    count, Ht, Wt, _ = frames.shape
    W, H = Wt if W is None else W, Ht if H is None else H
    n = count if n is None else n
    guard = Guard(poison=0xFF)
    good = max(int(G.load().kbe_gif_scratch_bytes(min(max(W, 1), Wt), min(max(H, 1), Ht), max(n, 1))), 8)
    scratch = guard.empty(((good + 7) // 8 * 8,), torch.uint8, 'cuda')
    out = torch.full((shift + cap + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    offsets = guard.full((max(n, 1) + 1,), -1, torch.int64, 'cuda')
    status = guard.full((1,), status_before, torch.int32, 'cuda')
    args = dict(frames_u8=pointers_of(frames, n), n_frames=n, W=W, H=H, stride_bytes=3 * Wt if stride is None else stride, flags=flags, dither=dither, delay_cs=delay_cs,
                lut=lut.data_ptr(), scratch=scratch.data_ptr(), out=out.data_ptr() + shift, cap=cap, offsets=offsets.data_ptr(), status=status.data_ptr(), stream=stream())
    if change:
        change(args)
    rc = G._raw('kbe_gif_encode', *args.values())
    torch.cuda.synchronize()
    guard.check()
    got = out.cpu().numpy()
    assert (got[:shift] == SENTINEL).all()
    return rc, offsets.cpu().tolist(), int(status.item()), got[shift:], bool((scratch == 0xFF).all())


def sizes_of(want):
    return np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()


def assert_units(frames, lut, want, room=333, **kw):
    """The device's units of `frames` are `want`, back to back; no byte in front of them or behind them is touched."""
    total = sum(len(s) for s in want)
    rc, offsets, status, buf, _ = run(on_device(frames), lut, total + room, **kw)
    assert rc == 0 and status == 0
    assert offsets == sizes_of(want)
    assert buf[:total].tobytes() == b''.join(want)
    assert (buf[total:] == SENTINEL).all()


def assert_case(name):
    """A case of the CPU suite, 1, 3 and 13 frames of different content (13: two launches, the offsets carry on), RGB and BGR, the dither off and on."""
    dev = on_device(gc.case_frames(name, 13))
    for flags in (0, gc.BGR):
        lut = on_device(gc.case_palette(name, flags)[1])
        for dither in (0, gc.DITHER):
            want = gc.case_twin(name, 13, flags, dither)[0]
            for n in (1, 3, 13):
                assert_units(dev[:n], lut, want[:n], flags=flags, dither=dither)
