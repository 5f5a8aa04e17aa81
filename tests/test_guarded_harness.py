"""The guard-and-poison harness (tests/guarded.py) checked on itself: plain torch writes, no kernel of the project.  On host memory
without a GPU; the same on device and pinned memory on the GPU box."""
import pytest
import torch

import guarded

DEVICES = ['cpu', pytest.param('cuda', marks=pytest.mark.gpu), pytest.param('pinned', marks=pytest.mark.gpu)]


def _kw(device):
    return dict(device='cpu', pin_memory=True) if device == 'pinned' else dict(device=device)


@pytest.mark.parametrize('device', DEVICES)
def test_an_untouched_run_is_clean_and_tensors_are_exact_and_poisoned(device):
    g = guarded.Guard(poison=0xFF)
    a = g.empty((3, 5, 7), torch.float32, **_kw(device))
    b = g.empty((0,), torch.uint8, **_kw(device))
    c = g.full((11,), 7, torch.int32, **_kw(device))
    d = g.empty((13,), torch.uint8, shift=3, **_kw(device))
    e = g.empty((2, 2), torch.float32, shift=4, **_kw(device))
    off = [t.data_ptr() - x.whole.data_ptr() for t, x in zip((a, b, c, d, e), g.allocations) if t.numel()]
    assert [v % 512 for v in off] == [0, 0, 3, 4], 'a tensor is as aligned as its allocation, or off by its shift'
    assert device == 'cpu' or a.data_ptr() % 512 == 0
    assert a.shape == (3, 5, 7) and a.is_contiguous() and bool(torch.isnan(a).all())
    assert b.numel() == 0 and c.tolist() == [7] * 11 and bool((d == 0xFF).all())
    sizes = [x.whole.numel() for x in g.allocations]
    assert sizes == [2 * guarded.GUARD + n for n in (420, 0, 44, 13 + 3, 16 + 4)], 'exactly the bytes asked for between two bands'
    assert guarded.GUARD % 512 == 0 and guarded.GUARD >= 4096
    a.fill_(1.0), c.fill_(-1), d.fill_(0), e.fill_(2.0)            # writing every byte of the tensors themselves is no finding
    g.check()
    assert bool((guarded.Guard(poison=0x00).empty((9,), torch.int32, **_kw(device)) == 0).all())


@pytest.mark.parametrize('device', DEVICES)
@pytest.mark.parametrize('band,index,offset', [('rear', 7 * 4, 0), ('rear', 7 * 4 + guarded.GUARD - 1, guarded.GUARD - 1), ('front', -1, -1), ('front', -guarded.GUARD, -guarded.GUARD)])
def test_one_byte_written_into_a_band_is_reported_with_its_call_site(device, band, index, offset):
    g = guarded.Guard()
    g.empty((5,), torch.float32, **_kw(device))
    t = g.empty((7,), torch.float32, **_kw(device))                 # <- the call site the report names
    g.full((3,), 0, torch.uint8, **_kw(device))
    alloc = g.allocations[1]
    alloc.whole[alloc.front + index] = 0                            # a torch indexing write of one byte, into the harness's own allocation
    with pytest.raises(AssertionError) as err:
        g.check()
    text = str(err.value)
    assert '%s band' % band in text and 'offset %d ' % offset in text and 'test_guarded_harness.py' in text and '(7,)' in text, text
    assert text.count('band of') == 1, 'only the touched allocation is reported'
    assert bool(torch.isnan(t).all())


def test_the_interception_of_the_binding_swaps_torch_for_the_block_only():
    from ken_burns_effect_amd import _native
    with guarded.Guard(poison=0x00) as g:
        assert _native.torch is not torch and _native.torch.float32 is torch.float32
        z = _native.torch.zeros(2, 3, dtype=torch.float32, device='cpu')
        f = _native.torch.full((4,), 0xA5, dtype=torch.uint8, device='cpu')
        e = _native.torch.empty(5, dtype=torch.int64, device='cpu')
        like = _native.torch.empty_like(z)
        assert z.shape == (2, 3) and f.tolist() == [0xA5] * 4 and e.tolist() == [0] * 5 and like.shape == z.shape
        assert len(g.allocations) == 4 and all('test_guarded_harness.py' in a.site for a in g.allocations)
    assert _native.torch is torch
    with pytest.raises(AssertionError, match='rear band'):
        with guarded.Guard() as g:
            t = _native.torch.empty(3, dtype=torch.uint8, device='cpu')
            g.allocations[0].whole[g.allocations[0].front + 3] = 1
    assert _native.torch is torch
