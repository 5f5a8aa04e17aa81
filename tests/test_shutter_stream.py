"""The shutter mean (include/kbe_shutter.h) without a GPU: csrc/kbe_shutter_block.h executed serially (tests/shutter_check.cpp) against the plain
definition and against the NumPy twin (tests/shutter_cases.py); the pinned bytes; where the samples lie on the path (shutter.sample_steps); the
binding (shutter.py) held to what tests/test_header_bindings.py holds the older headers to; every refusal of the entry on host memory; and the
command line's --shutter / --shutter-samples and Pipeline(shutter=, shutter_samples=)."""
import ctypes
import inspect
import os
import re
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest
from PIL import Image

import gif_cases as gc
import shutter_cases as sc
import test_header_bindings as thb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition ---------------------------------------------------------------------------
def test_the_packed_forms_are_the_plain_one():
    """shutter_check.cpp builds; for every S in 1..32 and every sum in 0..255 S the header's mean is (2 sum + S) / (2 S) and within 1/2 of
    sum / S, the multiply-high gives the same, the 16-bit lanes and the funnel shift give the plain bytes (all-255 dwords at S = 32 among
    them), and rows at every pair of classes modulo 16 are the plain form byte by byte."""
    m = re.search(r'brute: sums (\d+), plain mismatches (\d+), multiply-high mismatches (\d+), packed mismatches (\d+), realign mismatches (\d+), rows (\d+), row mismatches (\d+)', sc.ask('brute'))
    sums, plain, magic, packed, realign, rows, row_bad = (int(v) for v in m.groups())
    assert sums == sum(255 * S + 1 for S in range(1, 33)) and rows == 70 * 16 * 16
    assert (plain, magic, packed, realign, row_bad) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize('S', sc.SAMPLES)
@pytest.mark.parametrize('frame', sc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_header_is_the_twin(frame, S):
    """mean_row of csrc/kbe_shutter_block.h on the GPU suite's frames, source rows padded by 5 (every row at another alignment): the NumPy
    twin byte for byte, and a mean that no single sample would pass for."""
    W, H = frame
    samples, want = sc.samples_of(W, H, S), sc.twin_of(W, H, S)
    assert np.array_equal(sc.header_mean(samples, pad=5), want)
    if S > 1:
        assert sc.differing_share(samples, want) > 0.5
    else:
        assert np.array_equal(want, samples[:, 0])


def _flat(*values):
    """One output of 5 x 3 pixels whose samples are flat frames of these values."""
    return np.stack([np.full((3, 5, 3), v, np.uint8) for v in values])[None]


def test_the_pinned_bytes():
    for values, want in (((0, 1), 1), ((0, 0, 1), 0), ((0, 1, 1), 1), ((255,) * 32, 255), ((1, 0), 1), ((254, 255), 255), ((0, 255), 128), ((0,) * 31 + (16,), 1), ((0,) * 31 + (15,), 0)):
        for mean in (sc.twin_mean, sc.header_mean):
            assert (mean(_flat(*values)) == want).all(), (values, mean.__name__)
    photo = gc.photo_like(9, 11, 4)
    for S in (1, 2, 7, 32):                                     # S = 1 and S equal samples: the sample
        assert np.array_equal(sc.header_mean(np.stack([photo] * S)[None])[0], photo) and np.array_equal(sc.twin_mean(np.stack([photo] * S)[None])[0], photo)


# -- where the samples lie ----------------------------------------------------------------------
def test_sample_steps_of_the_issues_example():
    from ken_burns_effect_amd import shutter
    assert shutter.offsets(3) == [-1 / 3, 0.0, 1 / 3] and shutter.offsets(1) == [0.0] and shutter.offsets(2) == [-0.25, 0.25]
    for S in (1, 2, 5, 8, 32):
        o = shutter.offsets(S)
        assert len(o) == S and o == sorted(o) and -0.5 < o[0] and o[-1] < 0.5 and np.allclose(np.diff(o), 1.0 / S) and np.allclose(o, [-v for v in o[::-1]])
    got = shutter.sample_steps(np.linspace(0.0, 1.0, 5).tolist(), 0.5, 3)
    assert len(got) == 15
    for frame, want in ((0, (1 / 24, 0.0, 1 / 24)), (2, (0.5 - 1 / 24, 0.5, 0.5 + 1 / 24)), (4, (1.0 - 1 / 24, 1.0, 1.0 - 1 / 24))):
        assert np.abs(np.array(got[3 * frame:3 * frame + 3]) - np.array(want)).max() <= 1e-15, frame


def test_sample_steps_properties():
    from ken_burns_effect_amd import shutter
    uniform = np.linspace(0.0, 1.0, 7).tolist()
    uneven = [0.0, 0.05, 0.3, 0.31, 0.8, 1.0]
    # one sample, or a shutter that is not open: every step, `samples` times
    assert shutter.sample_steps(uniform, 0.7, 1) == uniform
    assert shutter.sample_steps(uneven, 0.0, 4) == [t for t in uneven for _ in range(4)]
    # no camera leaves the path
    for steps in (uniform, uneven, uneven[::-1], [0.2, 0.9]):
        got = shutter.sample_steps(steps, 1.0, 32)
        assert len(got) == 32 * len(steps) and min(got) >= min(steps) and max(got) <= max(steps)
    # a single step has all its samples on itself
    assert shutter.sample_steps([0.4], 1.0, 5) == [0.4] * 5
    # an interior frame: strictly increasing on an increasing path, symmetric about the step on uniform steps; never beyond half way to a neighbour
    for steps in (uniform, uneven):
        for S in (2, 3, 8):
            got = shutter.sample_steps(steps, 0.5, S)
            for i in range(1, len(steps) - 1):
                mine = got[S * i:S * i + S]
                assert all(a < b for a, b in zip(mine, mine[1:])), (steps, S, i)
                assert (steps[i - 1] + steps[i]) / 2 < mine[0] and mine[-1] < (steps[i] + steps[i + 1]) / 2
                if steps is uniform:
                    assert np.allclose([m - steps[i] for m in mine], [steps[i] - m for m in mine[::-1]], rtol=0, atol=1e-15)
    # the ends fold back: the first frame's samples lie towards the second step on both sides
    first = shutter.sample_steps(uneven, 1.0, 4)[:4]
    assert first == [first[3], first[2], first[2], first[3]] and all(0.0 < v < 0.05 for v in first)
    last = shutter.sample_steps(uneven, 1.0, 4)[-4:]
    assert last == [last[3], last[2], last[2], last[3]] and all(0.8 < v < 1.0 for v in last)


def test_the_shutter_is_a_small_record_and_is_checked():
    from ken_burns_effect_amd import shutter
    assert shutter.Shutter(0.5) == (0.5, 8) and shutter.Shutter(1, 4).samples == 4 and shutter.MAX_SAMPLES == 32
    assert shutter.checked((0.5,)) == shutter.Shutter(0.5, 8) and shutter.checked((0, 1)) == shutter.Shutter(0.0, 1) and shutter.checked((1, 32)) == shutter.Shutter(1.0, 32)
    for bad in ((-0.1, 8), (1.5, 8), (float('nan'), 8), (float('inf'), 8), (0.5, 0), (0.5, 33), (0.5, 2.5), ('wide', 8), (0.5, None)):
        with pytest.raises(ValueError, match='^shutter: '):
            shutter.checked(bad)
        with pytest.raises(ValueError, match='^shutter: '):
            shutter.sample_steps([0.0, 1.0], *bad)


# -- the binding -------------------------------------------------------------------------------
p, i = c_void_p, c_int
NULL_CALL = (None, 1, 2, 4, 4, 12, None, 12, None)
SHUTTER = thb.Binding(
    'shutter', 'kbe_shutter',
    # frames, n_out, samples, W, H, stride; out, out stride; stream
    {'kbe_shutter_abi_version': (c_int, []), 'kbe_shutter_mean_u8': (c_int, [p, i, i, i, i, i, p, i, p])},
    'kbe_shutter_abi_version', ['#define KBE_SHUTTER_ABI_VERSION 1\n'], ['KBE_SHUTTER_BGR'], {'ABI_VERSION': 1, 'MAX_SAMPLES': 32},
    [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n'), ('kbe_area.h', '#define KBE_AREA_ABI_VERSION 1\n'),
     ('kbe_crop_area.h', '#define KBE_CROP_AREA_ABI_VERSION 1\n'), ('kbe_dof.h', '#define KBE_DOF_ABI_VERSION 1\n')],
    ('kbe_shutter_mean_u8', NULL_CALL, 'kbe_shutter_mean_u8: null frames_u8'),
    ('kbe_shutter_mean_u8', None, lambda frames: ((frames, 1.0, 2, 4, 4, 12, frames, 12, None), (frames, 1, 2, 4, 4, 12, frames, c_size_t(12), None), (frames, 1, 2, 4, 4, 12, frames, 12))),
    [('kbe_shutter_abi_version', 0, (1,)), ('kbe_shutter_mean_u8', 9, NULL_CALL + (0,)), ('kbe_shutter_mean_u8', 9, NULL_CALL[:-1])],
    ['kbe_dof_u8', 'kbe_crop_area_u8', 'kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_shutter_mean_u8', lambda at: ((c_void_p * 4)(at, at + 1024, at + 2048, at + 3072), 2, 33, 16, 17, 48, (c_void_p * 2)(at + 4096, at + 5120), 48, None),
     'kbe_shutter_mean_u8 failed (-1): kbe_shutter_mean_u8: samples outside 1..32'),
    ['kbe_shutter_mean_u8'], set())
# what the other headers' modules declare: the lists this header must leave as they are
OTHERS = {'gif': list(thb.GIF.protos), 'area': list(thb.AREA.protos), 'crop_area': ['kbe_crop_area_abi_version', 'kbe_crop_area_u8'], 'dof': ['kbe_dof_abi_version', 'kbe_dof_u8']}


def test_the_header_parses_to_exactly_its_two_entries():
    thb.test_the_header_parses_to_exactly_its_entries(SHUTTER)
    from ken_burns_effect_amd import shutter
    assert list(shutter.prototypes()) == ['kbe_shutter_abi_version', 'kbe_shutter_mean_u8']


def test_the_library_exports_them_beside_the_others():
    import importlib
    thb.test_the_library_exports_them_with_the_headers_types(SHUTTER)
    from ken_burns_effect_amd import _native, shutter
    lib = shutter.load()
    assert lib is _native.load() and lib.kbe_shutter_abi_version() == 1 == shutter.ABI_VERSION
    for name, entries in OTHERS.items():
        module = importlib.import_module('ken_burns_effect_amd.' + name)
        assert module.load() is lib and getattr(lib, entries[0])() == 1


def test_the_older_headers_and_their_bindings_are_what_they_were():
    import importlib
    from ken_burns_effect_amd import _native, shutter
    b = SHUTTER
    shutter.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for name, entries in OTHERS.items():
        other = importlib.import_module('ken_burns_effect_amd.' + name)
        assert list(other.prototypes()) == entries and other.ABI_VERSION == 1
    # shutter.py is the only module of the package whose text names the header's prefix, and it names no entry of another header
    package = os.path.dirname(shutter.__file__)
    naming = [name for name in sorted(os.listdir(package)) if name.endswith('.py') and b.prefix in open(os.path.join(package, name)).read()]
    assert naming == ['shutter.py']
    with open(shutter.__file__) as f:
        text = f.read()
    foreign = set(_native.SYMBOLS) | {entry for entries in OTHERS.values() for entry in entries}
    assert not [entry for entry in sorted(foreign) if entry in text]
    name, args, text = b.null_call
    assert shutter._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    thb.test_ctypes_refuses_a_wrong_call_before_it_is_made(SHUTTER)


def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused():
    thb.test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(SHUTTER)


def test_call_reports_a_refusal_with_the_librarys_text():
    thb.test_call_reports_a_refusal_with_the_librarys_text(SHUTTER)


def test_every_call_site_passes_the_headers_number_of_arguments():
    thb.test_every_call_site_passes_the_headers_number_of_arguments(SHUTTER)


# (frames of 16 x 17 at a stride of 48: 816 bytes.  The four sources lie at 0, 2048, 4096 and 6144 of 32 KiB of host memory, the two outputs
# at 10240 and 12288; (a, b): outputs moved there, None: as it was)
REFUSED = {'null frames': (dict(frames_u8=None), 'null frames_u8'), 'null out': (dict(out_u8=None), 'null out_u8'), 'n = 0': (dict(n_out=0), 'n_out < 1'),
           'n = -1': (dict(n_out=-1), 'n_out < 1'), 'samples 0': (dict(samples=0), 'samples outside 1..32'), 'samples 33': (dict(samples=33), 'samples outside 1..32'),
           'W = 0': (dict(W=0), 'W or H outside 1..65535'), 'H = 65536': (dict(H=65536), 'W or H outside 1..65535'), 'stride': (dict(stride_bytes=47), 'stride_bytes < 3 W'),
           'out stride': (dict(out_stride_bytes=47), 'out_stride_bytes < 3 W'), 'null frame 3': (dict(frames_u8=3), 'null element of frames_u8'),
           'null frame 0': (dict(frames_u8=0), 'null element of frames_u8'), 'null output 1': (dict(out_u8=1), 'null element of out_u8'),
           'in place': (dict(out_u8=(0, None)), 'an element of out_u8 overlaps a source frame'),
           'onto the other outputs source': (dict(out_u8=(6144, None)), 'an element of out_u8 overlaps a source frame'),
           'one byte into the next source': (dict(out_u8=(2048 - 815, None)), 'an element of out_u8 overlaps a source frame'),
           'the last byte of the last source': (dict(out_u8=(None, 6144 + 815)), 'an element of out_u8 overlaps a source frame'),
           'one outputs last byte on the others first': (dict(out_u8=(12288 - 815, None)), 'an element of out_u8 overlaps another output'),
           'the same output twice': (dict(out_u8=(None, 10240)), 'an element of out_u8 overlaps another output'),
           # repeated sources pass every check of the sources: the refusal is the last check's
           'repeated sources': (dict(repeat=True, out_u8=(None, 10240 + 815)), 'an element of out_u8 overlaps another output')}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_refusal_texts(what):
    """Every argument is refused before anything is enqueued, on host memory no kernel could touch, and the text names the entry and the argument."""
    from ken_burns_effect_amd import _native, shutter
    memory = (ctypes.c_uint64 * 4096)()
    at = ctypes.addressof(memory)
    args = dict(frames_u8=(c_void_p * 4)(at, at + 2048, at + 4096, at + 6144), n_out=2, samples=2, W=16, H=17, stride_bytes=48,
                out_u8=(c_void_p * 2)(at + 10240, at + 12288), out_stride_bytes=48, stream=None)
    change, text = REFUSED[what]
    for key, value in change.items():
        if key == 'repeat':
            args['frames_u8'] = (c_void_p * 4)(at, at + 2048, at + 2048, at)
        elif key in ('frames_u8', 'out_u8') and isinstance(value, int):
            args[key][value] = None
        elif key == 'out_u8' and isinstance(value, tuple):
            for k in (0, 1):
                if value[k] is not None:
                    args[key][k] = at + value[k]
        else:
            args[key] = value
    assert shutter._raw('kbe_shutter_mean_u8', *args.values()) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_shutter_mean_u8: ' + text
    assert not any(memory)


def test_mean_refuses_what_is_no_tensor_on_the_gpu():
    import torch
    from ken_burns_effect_amd import _native, shutter
    for bad, S in ((torch.zeros(4, 8, 8, 3, dtype=torch.uint8), 2), (np.zeros((4, 8, 8, 3), np.uint8), 2), (torch.zeros(4, 8, 8, 3), 2), (torch.zeros(8, 8, 3, dtype=torch.uint8), 1)):
        with pytest.raises(_native.KbeError, match=r'shutter\.mean'):
            shutter.mean(bad, S)


# -- the command line and Pipeline ---------------------------------------------------------------
ENV = ('KBE_SHUTTER', 'KBE_SHUTTER_SAMPLES')
CLI_REFUSALS = ((['--shutter', '0'], r'^--shutter 0: the shutter \(KBE_SHUTTER, --shutter\): the share of a frame interval it is open, a finite number above 0 and at most 1$'),
                (['--shutter', '1.5'], r'^--shutter 1\.5: the shutter'), (['--shutter', 'nan'], r'^--shutter nan: the shutter'), (['--shutter', '-0.5'], r'^--shutter -0\.5: the shutter'),
                (['--shutter', 'open'], r'^--shutter open: the shutter'), (['--shutter-samples', '4'], r'^--shutter-samples 4: only with --shutter$'),
                (['--shutter', '0.5', '--shutter-samples', '1'], r"^--shutter-samples 1: the shutter's samples \(KBE_SHUTTER_SAMPLES, --shutter-samples\): a whole number, 2\.\.32$"),
                (['--shutter', '0.5', '--shutter-samples', '33'], r"^--shutter-samples 33: the shutter's samples"), (['--shutter', '0.5', '--shutter-samples', '2.5'], r"^--shutter-samples 2\.5: the shutter's samples"))


def test_the_command_line_takes_and_refuses_the_shutter(monkeypatch):
    from ken_burns_effect_amd import kbe
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    cfg = kbe.parse([])[0]
    assert cfg['shutter'] is None and cfg['shutter-samples'] is None
    cfg = kbe.parse(['--shutter', '0.5'])[0]
    assert cfg['shutter'] == 0.5 and cfg['shutter-samples'] == 8
    cfg = kbe.parse(['--shutter', '1', '--shutter-samples', '32', '--width', '64', '--gif', '--gif-fps', '12.5', '--dolly', '--aperture', '6'])[0]
    assert cfg['shutter'] == 1.0 and cfg['shutter-samples'] == 32 and cfg['width'] == 64 and cfg['gif'] and cfg['dolly'] and cfg['aperture'] == 6.0
    for argv, text in CLI_REFUSALS:
        with pytest.raises(SystemExit, match=text):
            kbe.parse(argv)
    assert '--shutter F' in kbe.__doc__ and '--shutter-samples S' in kbe.__doc__


def test_shutter_request(monkeypatch):
    from ken_burns_effect_amd import pipeline, shutter
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    assert pipeline.shutter_request() is None and pipeline.shutter_request(0.5) == shutter.Shutter(0.5, 8) and pipeline.shutter_request('0.25', '4') == (0.25, 4)
    assert pipeline.shutter_request(1, 2) == (1.0, 2) and pipeline.shutter_request(1e-3, 32) == (1e-3, 32)
    for bad in (0, 0.0, -1, 1.5, float('nan'), float('inf'), 'open', '0'):
        with pytest.raises(ValueError, match=r'^the shutter \(KBE_SHUTTER, --shutter\): the share of a frame interval it is open, a finite number above 0 and at most 1$'):
            pipeline.shutter_request(bad)
    for bad in (1, 33, 0, -4, 2.5, 'many', '1'):
        with pytest.raises(ValueError, match=r"^the shutter's samples \(KBE_SHUTTER_SAMPLES, --shutter-samples\): a whole number, 2\.\.32$"):
            pipeline.shutter_request(0.5, bad)
    with pytest.raises(ValueError, match=r'^shutter_samples \(KBE_SHUTTER_SAMPLES, --shutter-samples\): only with a shutter \(KBE_SHUTTER, --shutter\)$'):
        pipeline.shutter_request(None, 4)
    monkeypatch.setenv('KBE_SHUTTER_SAMPLES', '4')
    with pytest.raises(ValueError, match='only with a shutter'):
        pipeline.shutter_request()
    monkeypatch.setenv('KBE_SHUTTER', '0.75')
    assert pipeline.shutter_request() == (0.75, 4) and pipeline.shutter_request(0.5) == (0.5, 4) and pipeline.shutter_request(None, 16) == (0.75, 16)
    monkeypatch.setenv('KBE_SHUTTER', '2')
    with pytest.raises(ValueError, match='KBE_SHUTTER'):
        pipeline.shutter_request()


def _stub(P, calls, **settings):
    import torch

    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = False, False, 2, {}, None, torch.device('cpu')
            for name, value in settings.items():
                setattr(self, name, value)

        def estimate(self, tensorImage):
            calls.append('estimate')
            raise AssertionError('a network ran')
    return Stub()


def test_a_shutter_that_cannot_be_is_refused_before_a_network_runs(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import kbe, pipeline, synthetic
    for name in ENV + ('KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_WIDTH', 'KBE_GIF'):
        monkeypatch.delenv(name, raising=False)
    calls = []
    monkeypatch.setattr(pipeline.common, 'process_kenburns', lambda *a, **k: calls.append('render'))
    image = torch.zeros(1, 3, 48, 64)
    ofrom, oto = synthetic.default_windows(48, 64)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}
    for settings, text in ((dict(shutter=0), 'above 0 and at most 1'), (dict(shutter=1.5), 'above 0 and at most 1'), (dict(shutter=float('nan')), 'above 0 and at most 1'),
                           (dict(shutter_samples=4), 'only with a shutter'), (dict(shutter=0.5, shutter_samples=1), 'a whole number, 2..32'),
                           (dict(shutter=0.5, shutter_samples=33), 'a whole number, 2..32')):
        with pytest.raises(ValueError, match=text):
            _stub(pipeline, calls, **settings)(image, zoom, str(tmp_path / 'out'))
    monkeypatch.setenv('KBE_SHUTTER_SAMPLES', '4')
    with pytest.raises(ValueError, match='only with a shutter'):
        _stub(pipeline, calls)(image, zoom, None)
    monkeypatch.setenv('KBE_SHUTTER', '0')
    with pytest.raises(ValueError, match='above 0 and at most 1'):
        _stub(pipeline, calls)(image, zoom, None)
    assert calls == [] and not (tmp_path / 'out').exists()
    # the command line: before Pipeline is built
    for name in ENV:
        monkeypatch.delenv(name)
    built = []
    monkeypatch.setattr(pipeline.Pipeline, '__init__', lambda self, *a, **k: built.append(k))
    path = str(tmp_path / 'in.png')
    Image.fromarray(gc.photo_like(48, 64, 1)).save(path)
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        for argv, text in CLI_REFUSALS:
            with pytest.raises(SystemExit, match=text):
                kbe.main(['--in', path, '--out', str(tmp_path / 'out')] + argv)
    finally:
        torch.set_grad_enabled(grad)
    assert built == [] and not (tmp_path / 'out').exists()


def test_the_pipeline_passes_a_shutter_only_when_there_is_one(monkeypatch):
    """Without a shutter process_kenburns is called with exactly the arguments it had; with one, it gets the Shutter, beside a width and a lens."""
    import torch
    from ken_burns_effect_amd import dof, pipeline, shutter, synthetic
    for name in ENV + ('KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_PNG', 'KBE_JPEG'):
        monkeypatch.delenv(name, raising=False)
    seen = []

    def kenburns(*args, **kw):
        seen.append(kw)
        size = kw.get('out_size', (64, 48))
        return [np.zeros((size[1], size[0], 3), np.uint8) for _ in range(2)]
    monkeypatch.setattr(pipeline.common, 'process_kenburns', kenburns)
    ofrom, oto = synthetic.default_windows(48, 64)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}

    def run(**settings):
        stub = _stub(pipeline, [], **settings)
        stub.objectCommon = {'tensorRawDepth': torch.full((1, 1, 48, 64), 200.0)}
        stub.estimate = lambda tensorImage: None
        return stub(torch.zeros(1, 3, 48, 64), zoom, None)
    assert [f.shape for f in run()] == [(48, 64, 3)] * 2 and seen == [{'keep_on_device': False}]
    run(shutter=0.5)
    assert seen[1] == {'keep_on_device': False, 'shutter': shutter.Shutter(0.5, 8)}
    run(shutter='0.25', shutter_samples=4, width=32, aperture=6)
    assert seen[2] == {'keep_on_device': False, 'out_size': (32, 24), 'lens': dof.Lens(200.0, 200.0, 6.0, 16), 'shutter': shutter.Shutter(0.25, 4)}
    monkeypatch.setenv('KBE_SHUTTER', '1')
    monkeypatch.setenv('KBE_SHUTTER_SAMPLES', '2')
    run()
    assert seen[3] == {'keep_on_device': False, 'shutter': shutter.Shutter(1.0, 2)}


def test_process_kenburns_and_render_frames_take_a_shutter():
    from ken_burns_effect_amd import common, sharding
    assert inspect.signature(common.render_frames).parameters['shutter'].default is None
    assert inspect.signature(common.process_kenburns).parameters['shutter'].default is None
    assert inspect.signature(common._render_lens).parameters['focus'].default is None
    with open(sharding.__file__) as f:
        assert 'shutter' not in f.read()                                    # (the sharded path is out of scope: it does not take the argument)
    with pytest.raises(ValueError, match='^shutter: samples'):
        common.render_frames([], {}, None, shutter=(0.5, 33))
    with pytest.raises(ValueError, match='^shutter: fraction'):
        common.render_frames([], {}, None, shutter=(1.5, 4))
    with pytest.raises(ValueError, match='no whole number of frames of 4 samples'):
        common.render_frames([(1.0, (0.0, 0.0, 0.0))] * 6, {}, None, shutter=(0.5, 4))
