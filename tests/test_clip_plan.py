"""What a Pipeline decides on the host before any network runs, on bare stubs at 64 x 48 with two steps and no GPU: __call__ and render ask
process_kenburns for the same clip, and of two faulty options the one that is looked at first is the one reported."""
import os

import pytest

W, H = 64, 48


def _stub(P, seen, **options):
    import torch

    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = False, False, 2, {}, None, torch.device('cpu')
            for name, value in options.items():
                setattr(self, name, value)

        def estimate(self, tensorImage):
            seen.append('estimate')
            # (a ramp: every depth is its own pixel's, so the median of a 5 x 5 window inside the image is its centre's)
            self.objectCommon['tensorRawDepth'] = torch.arange(1, W * H + 1, dtype=torch.float32).reshape(1, 1, H, W)
    return Stub()


@pytest.fixture
def P(monkeypatch):
    from ken_burns_effect_amd import pipeline
    for name in [n for n in os.environ if n.startswith('KBE_')]:
        monkeypatch.delenv(name)
    return pipeline


@pytest.fixture
def zoom(P):
    from ken_burns_effect_amd import synthetic
    ofrom, oto = synthetic.default_windows(H, W)
    settings = {'objectFrom': ofrom, 'objectTo': oto}
    assert P.common.crop_size(settings) == (57, 43)
    return settings


def _depth(u, v):
    return float(1 + v * W + u)


def test_call_and_render_ask_for_the_same_clip(P, zoom, monkeypatch):
    import numpy as np
    import torch
    from ken_burns_effect_amd import dof
    from ken_burns_effect_amd.shutter import Shutter
    seen = []

    def kenburns(settings, common, inpaint, keep_on_device=False, **keywords):
        seen.append((settings, keywords, keep_on_device))
        w, h = keywords.get('out_size', (W, H))
        frames = np.zeros((2, h, w, 3), np.uint8)
        return torch.from_numpy(frames) if keep_on_device else list(frames)
    monkeypatch.setattr(P.common, 'process_kenburns', kenburns)
    image = torch.zeros(1, 3, H, W)
    lens = dof.Lens(_depth(10, 11), _depth(40, 30), 3.0)
    # (without a focus: the end window's centre, rounded to its pixel, which lies more than two pixels inside the image)
    centre = _depth(int(zoom['objectTo']['dblCenterU'] + 0.5), int(zoom['objectTo']['dblCenterV'] + 0.5))
    rows = [({}, {}),
            (dict(width=32), {'out_size': (32, 24)}),
            (dict(width=128, enlarge=True), {'enlarge': True, 'out_size': (128, 96)}),
            (dict(aperture=3, focus=(10, 11), focus_to=(40, 30)), {'lens': lens}),
            (dict(shutter=0.5, shutter_samples=4), {'shutter': Shutter(0.5, 4)}),
            (dict(width=32, aperture=2, shutter=1), {'out_size': (32, 24), 'lens': dof.Lens(centre, centre, 2.0), 'shutter': Shutter(1.0)})]
    for options, keywords in rows:
        del seen[:]
        size = keywords.get('out_size', (W, H))
        called = _stub(P, seen, **options)(image, zoom, None)
        assert [f.shape for f in called] == [(size[1], size[0], 3)] * 2
        rendered = _stub(P, seen, **options).render(image, zoom)
        assert tuple(rendered.shape) == (2, size[1], size[0], 3)
        assert [s for s in seen if s == 'estimate'] == ['estimate'] * 2 and len(seen) == 4
        (settings, asked, kept), (settings_r, asked_r, kept_r) = seen[1], seen[3]
        assert settings == settings_r and settings == {'dblSteps': [0.0, 1.0], 'objectFrom': zoom['objectFrom'], 'objectTo': zoom['objectTo'], 'boolInpaint': True, 'dolly': False}
        assert asked == asked_r == keywords and set(asked) == set(keywords), options
        assert (kept, kept_r) == (False, True)


FAULTS = [(dict(gif=True, gif_width=0, width=0), r"^the GIF's width \(KBE_GIF_WIDTH, --gif-width\)"),
          (dict(width=999, aperture=-1), r'^width 999: the crop is 57 pixels wide'),
          (dict(gif=True, gif_width=40, width=32, aperture=-1), r'^a GIF 40 pixels wide from frames 32 wide'),
          (dict(aperture=-1, shutter=9), r'^the aperture \(KBE_APERTURE, --aperture\)'),
          (dict(shutter=9, caption=''), r'^the shutter \(KBE_SHUTTER, --shutter\)'),
          (dict(caption='', look='warm'), r"^--caption '': an empty caption"),
          (dict(look='warm', sharpen='9'), r'^--look warm')]


def test_the_first_fault_is_the_one_reported(P, zoom, monkeypatch, tmp_path):
    import torch
    seen = []
    monkeypatch.setattr(P.common, 'process_kenburns', lambda *a, **k: seen.append('render'))
    image = torch.zeros(1, 3, H, W)
    out = str(tmp_path / 'out')
    for options, match in FAULTS:
        with pytest.raises(ValueError, match=match):
            _stub(P, seen, **options)(image, zoom, out)
        if 'gif' not in options:
            with pytest.raises(ValueError, match=match):
                _stub(P, seen, **options)(image, zoom, None)
            with pytest.raises(ValueError, match=match):
                _stub(P, seen, **options).render(image, zoom)
    assert seen == [] and not (tmp_path / 'out').exists()
