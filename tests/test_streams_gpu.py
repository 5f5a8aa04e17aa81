"""Streams: every device entry on a non-blocking side stream behind a delay (the method: tests/stream_gpu.py; the cases and their bars:
tests/stream_cases.py).  The rest of the GPU suite calls everything on torch's default stream, where a launch, memset or copy on the wrong
stream and a lane that is not forked from or joined to the caller's stream change nothing.  No value here is held against the oracle: `want` is
the same call on the default stream, which the rest of the suite holds to it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dof_cases as dc
import gif_cases as gc
import mjpeg_cases as mc
import stream_cases as sc
import stream_gpu as sg
import test_hip_guarded as hg
from test_hip_guarded import CAMERA, CAMERAS, K, glue_calls, pipelined, stream, void      # noqa: F401 (K: the fixture)
from test_hip_parity import _scene

pytestmark = pytest.mark.gpu

F, BL = float(hg.F), float(hg.BL)


def ids(group):
    return [c.name for c in sc.cases_of(group)]


# ---------------------------------------------------------------------------------------
# a. glue, stage and network entries: test_hip_guarded.glue_calls' thunks, their input tensors refilled in place
# ---------------------------------------------------------------------------------------

def selftest_calls(K, seed=0):
    gen = torch.Generator().manual_seed(41 + seed)
    z = (torch.rand(1000, generator=gen) * 900 + 100).cuda()
    num, den = torch.randn(1000, generator=gen).cuda(), (torch.rand(1000, generator=gen) + 0.5).cuda()
    return [('selftest_err', lambda: K.selftest_err(z, F, BL), True), ('selftest_division', lambda: K.selftest_division(num, den), True)]


def closure_of(thunk):
    """(the tensors, everything else) a thunk of glue_calls reads, by the names glue_calls gives them."""
    cells = dict(zip(thunk.__code__.co_freevars, [c.cell_contents for c in thunk.__closure__ or ()]))
    return {k: v for k, v in cells.items() if torch.is_tensor(v)}, {k: v for k, v in cells.items() if not torch.is_tensor(v) and not callable(v) and k != 'K'}


@functools.lru_cache(maxsize=None)
def glue_sets(K, shape):
    """{name: (the thunk on the buffers, exact?, the buffers by name, their right values, their decoy values)} of one shape: the right set is
    glue_calls' own, the buffers are a second set of another seed, whose first contents are the decoy."""
    made = {}
    right = glue_calls(K, *shape) + selftest_calls(K)
    buffers = glue_calls(K, *shape, seed=1) + selftest_calls(K, seed=1)
    torch.cuda.synchronize()
    for (name, thunk_r, exact), (name_b, thunk_b, _) in zip(right, buffers):
        (tr, rest_r), (tb, rest_b) = closure_of(thunk_r), closure_of(thunk_b)
        assert name == name_b and list(tr) == list(tb) and repr(rest_r) == repr(rest_b), name
        made[name] = (thunk_b, exact, list(tb.values()), [t.clone() for t in tr.values()], [t.clone() for t in tb.values()])
    return made


GLUE_CASES = [(c.name, sc.GLUE_SHAPE) for c in sc.cases_of('glue')] + [(name, sc.VECTOR_SHAPE) for name in sc.VECTOR_THUNKS]


@pytest.mark.parametrize('name,shape', GLUE_CASES, ids=['%s-%s' % (n, 'x'.join(map(str, s))) for n, s in GLUE_CASES])
def test_glue_and_network_entries_on_a_side_stream(K, name, shape):
    """Every K. wrapper of csrc/kbe_hip.hip (the 33 thunks of test_hip_guarded.glue_calls, and the two self-tests) at (2,3,7,9), kbe_bias_act also
    at (1,5,12,20) -- k_bias_act<true> --: the thunk's own input tensors hold the decoy and are refilled behind the delay; the outputs and the
    scratch are the wrapper's fresh allocations on the side stream."""
    case = sc.case('glue', name)
    thunk, exact, buffers, right, decoy = glue_sets(K, shape)[name]
    assert exact == (case.bar == 'bits'), 'the table states glue_calls\' own bar'
    # (without a mask every window is valid: the second output of that call is ones whatever its input)
    sg.hold('%s at %s' % (name, shape), case.bar, buffers, right, decoy, thunk, differ_in=[0] if name == 'pconv_epilogue no mask' else None)


def test_the_table_names_every_thunk_of_glue_calls(K):
    names = [name for name, _, _ in glue_calls(K, *sc.GLUE_SHAPE)]
    assert len(names) == 33 and set(names) <= set(sc.GLUE), set(names) - set(sc.GLUE)


# ---------------------------------------------------------------------------------------
# b. kbe_render_pointcloud, kbe_degrid_serial from fp32 and kbe_zkeys_clear through the C ABI: the caller owns zkeys, zee and acc
# ---------------------------------------------------------------------------------------

def splat_inputs(K, seed, B, C, H, W):
    gen = torch.Generator().manual_seed(seed)
    depth = (torch.rand(B, 1, H, W, generator=gen) * 300 + 600).cuda()
    points = K.shift_points(K.depth_to_points(depth, F).view(B, 3, H * W).contiguous(), [3.25, -1.5, -12.0])
    return points, torch.rand(B, C, H * W, generator=gen).cuda()


@pytest.mark.parametrize('name', ids('abi'))
def test_entries_with_caller_owned_scratch_on_a_side_stream(K, name):
    """At the C-ABI level the z keys, the z-buffer and the sums are the caller's: they hold what the decoy's call left, and get it back behind the
    delay -- a key clear, the memset of `acc` or the copy of kbe_degrid_serial's fp32 input on another stream is undone or reads the decoy."""
    case = sc.case('abi', name)
    B, C, H, W = 2, 4, 7, 9
    N = H * W
    (p_r, d_r), (p_d, d_d) = splat_inputs(K, 1, B, C, H, W), splat_inputs(K, 2, B, C, H, W)
    points, data = p_d.clone(), d_d.clone()
    zkeys = torch.zeros(B * N, dtype=torch.int32, device='cuda')
    zee, acc = torch.zeros(B * N, device='cuda'), torch.zeros(B * (C + 1) * N, device='cuda')
    render, existing = torch.zeros(B, C, H, W, device='cuda'), torch.zeros(B, 1, H, W, device='cuda')
    if name == 'render_pointcloud':
        def call():
            K._call('kbe_render_pointcloud', void(points), void(data), B, N, C, W, H, F, BL, void(zkeys), void(zee), void(acc), void(render), void(existing), stream())
            return render, existing
        sg.hold(name, case.bar, [points, data], [p_r, d_r], [p_d, d_d], call, written=lambda: [zkeys, zee, acc, render, existing])
    elif name == 'degrid_serial from fp32':
        pre_r, pre_d = (K.zkeys_decode(K.zsplat(p, W, H, F, BL)[0]).reshape(-1) for p in (p_r, p_d))
        pre = pre_d.clone()

        def call():
            K._call('kbe_degrid_serial', None, void(pre), B, W, H, void(zee), stream())
            return zee
        sg.hold(name, case.bar, [pre], [pre_r], [pre_d], call, written=lambda: [zee])
    else:
        # the clear's result does not depend on an input: what it has to clear is the decoy -- the keys of a z-splat
        splat = K.zsplat(p_d, W, H, F, BL)[0].reshape(-1)

        def call():
            K._call('kbe_zkeys_clear', void(zkeys), zkeys.numel(), stream())
            return zkeys
        got, want = sg.hold(name, case.bar, [], [], [], call, written=lambda: [zkeys], dirty=lambda: zkeys.copy_(splat), differ_in=[])
        assert (splat.cpu().numpy() != want[0]).mean() >= 0.1, 'the keys the clear is undone to differ from cleared ones'


# ---------------------------------------------------------------------------------------
# c. the frame entries
# ---------------------------------------------------------------------------------------

def raster_cloud(H, W, seed):
    """test_hip_guarded.cloud_of('raster') with a seed: a point per pixel, (points [1,3,N], image [1,3,N], depth [1,1,N]) on the device."""
    g0 = torch.Generator().manual_seed(seed * 1000 + H * 131 + W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    z = 700.0 + 200.0 * torch.rand(H, W, generator=g0)
    pts = torch.stack([(xs - W / 2 + 0.5) * z / 512.0, (ys - H / 2 + 0.5) * z / 512.0, z])
    return [t.contiguous().cuda() for t in (pts.reshape(1, 3, -1), torch.rand(1, 3, H * W, generator=g0), z.reshape(1, 1, -1))]


def packed_of(K, cloud, H, W, near):
    return K.prepare_cloud(*[t.clone() for t in cloud], W, H, near_depth=near)['packed'].clone()


@functools.lru_cache(maxsize=None)
def raster_scene(K, H, W):
    """A resident cloud whose tensors (and packed form) are the buffers, with the right and the decoy values of both.  near_depth: the nearer
    of the two clouds', so that the lists the frames of a group share hold for either."""
    right, decoy = raster_cloud(H, W, 1), raster_cloud(H, W, 2)
    near = float(min(right[2].min(), decoy[2].min()))
    buffers = [t.clone() for t in decoy]
    state = K.prepare_cloud(*buffers, W, H, near_depth=near)
    assert state['fused'] and all(state[k].data_ptr() == b.data_ptr() for k, b in zip(('points', 'image', 'depth'), buffers)), 'the state reads the buffers in place'
    made = dict(state=state, buffers=buffers, right=right, decoy=decoy, packed=[state['packed']], packed_right=[packed_of(K, right, H, W, near)],
                packed_decoy=[packed_of(K, decoy, H, W, near)])
    torch.cuda.synchronize()
    return made


def scratch_of(state, *more):
    return lambda: [state[k] for k in ('scratch', 'scratch_groups', 'stage') if k in state] + list(more)


class Handed:
    """What test_hip_guarded.pipelined asks a Guard for: here the caller's own frames buffer, in pieces."""

    def __init__(self, frames):
        self.frames, self.at = frames, 0

    def empty(self, shape, dtype, device, shift=0):
        self.at += shape[0]
        return self.frames[self.at - shape[0]:self.at]


FRAME_CASES = [(c.name.rsplit(' ', 1)[0], tuple(int(v) for v in c.name.rsplit(' ', 1)[1].split('x'))) for c in sc.cases_of('frame')]


@pytest.mark.parametrize('kind,size', FRAME_CASES, ids=ids('frame'))
def test_frame_entries_on_a_side_stream(K, kind, size):
    """kbe_frame_scratch_init and _init_sets (each followed by a frame on the set it initialised: the sets hold a projection's z-buffer and
    buckets, a valid call's, which the decoy left and which they get back behind the delay), kbe_cloud_pack, one frame on the fused, bucket and
    generic routes with every optional output, the three group entries over 5 frames (the last pipelined over two launches) and
    kbe_render_pointcloud_tiled, on a raster with an odd pixel count and on one of whole tiles.  On the fused routes the packed cloud is what is
    swapped, elsewhere points, image and depth; the scratch sets get the decoy's snapshot back behind the delay."""
    H, W = size
    case = sc.case('frame', '%s %dx%d' % (kind, H, W))
    sn = raster_scene(K, H, W)
    state, N = sn['state'], H * W
    cloud, packed = (sn['buffers'], sn['right'], sn['decoy']), (sn['packed'], sn['packed_right'], sn['packed_decoy'])
    frame = torch.zeros(H, W, 3, dtype=torch.uint8, device='cuda')
    frames = torch.zeros(5, H, W, 3, dtype=torch.uint8, device='cuda')
    what = case.name
    if kind in ('scratch_init', 'scratch_init_sets'):
        stride = int(K.lib.kbe_video_scratch_stride(W, H, N))
        sets = torch.zeros(2 * stride if kind == 'scratch_init_sets' else int(K.lib.kbe_frame_scratch_bytes(W, H, N)), dtype=torch.uint8, device='cuda')
        mine = sets[stride:] if kind == 'scratch_init_sets' else sets
        on_mine = dict(state, scratch=mine)
        pts, img, dep = sn['buffers']

        def call():
            if kind == 'scratch_init':
                K._call('kbe_frame_scratch_init', void(sets), W, H, stream())
                K._call('kbe_render_frame', void(pts), void(img), void(dep), N, W, H, F, BL, (ctypes.c_float * 3)(*CAMERA), void(mine), void(frame), None, None, None, None, stream())
            else:
                K._call('kbe_frame_scratch_init_sets', void(sets), stride, 2, W, H, stream())
                K.render_frame(on_mine, CAMERA, F, BL, out=frame, fused=False)
            return frame
        # (the projection launch alone -- include/kbe.h: it leaves the z-buffer splatted and the buckets filled, which is what the init has to undo)
        sg.hold(what, case.bar, *cloud, call, written=lambda: [sets, frame], dirty=lambda: K.render_frame(on_mine, CAMERA, F, BL, out=frame, fused=False, stages=1))
    elif kind == 'cloud_pack':
        mine = torch.zeros_like(state['packed'])
        on_mine = dict(state, packed=mine)
        pts, img, dep = sn['buffers']

        def call():
            K._call('kbe_cloud_pack', void(pts), void(img), void(dep), N, W, H, state['cloud_focal'], state['raster_w'], state['raster_n'], void(mine), stream())
            return K.render_frame(on_mine, CAMERA, F, BL, out=frame, fused=True)
        sg.hold(what, case.bar, *cloud, call, written=scratch_of(state, mine, frame))
    elif kind in ('one frame fused', 'one frame bucket'):
        outs = {'zee_pre_f32': torch.zeros(N, device='cuda'), 'zee_f32': torch.zeros(N, device='cuda'), 'existing_f32': torch.zeros(N, device='cuda'),
                'render_f32': torch.zeros(4, H, W, device='cuda')}

        def call():
            K.render_frame(state, CAMERA, F, BL, out=frame, fused=kind == 'one frame fused', **outs)
            return (frame,) + tuple(outs.values())
        sg.hold(what, case.bar, *(packed if kind == 'one frame fused' else cloud), call, written=scratch_of(state, frame, *outs.values()))
    elif kind == 'one frame generic':
        generic = dict(state, generic=True)
        generic.pop('generic_data', None)

        def call():
            generic.pop('generic_data', None)              # (the route's own copy of image and depth: made again from the buffers, on the stream of the call)
            return K.render_video(generic, [(F, CAMERA)], BL, host_out=frames[:1])
        sg.hold(what, case.bar, *cloud, call, written=lambda: [frames])
    elif kind == 'group':
        def call():
            K.render_frame_group(state, CAMERAS[:4], BL, frames[:4])
            K.render_frame_group(state, CAMERAS[4:5], BL, frames[4:])
            return frames
        sg.hold(what, case.bar, *cloud, call, written=scratch_of(state, frames))
    elif kind == 'group_fused':
        sg.hold(what, case.bar, *packed, lambda: K.render_frame_group_fused(state, CAMERAS[:5], BL, frames), written=scratch_of(state, frames))
    elif kind == 'group_ahead':
        def call():
            pipelined(K, state, Handed(frames), [3, 2], H, W)
            return frames
        sg.hold(what, case.bar, *packed, call, written=scratch_of(state, frames))
    else:
        assert kind == 'render_pointcloud_tiled'
        moved = [K.shift_points(c[0], CAMERA) for c in (sn['right'], sn['decoy'])]
        data = [torch.cat([c[1], c[2]], 1).contiguous() for c in (sn['right'], sn['decoy'])]
        pts, dat = moved[1].clone(), data[1].clone()
        sg.hold(what, case.bar, [pts, dat], [moved[0], data[0]], [moved[1], data[1]], lambda: K.render_pointcloud(pts, dat, W, H, F, BL, tiled=True),
                written=lambda: list(K._tiled_scratch.values()))


# ---------------------------------------------------------------------------------------
# d. kbe_render_video
# ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def video_scene(H, W, n_frames):
    """(cameras, crop, the right cloud, the decoy cloud, the nearer of their nearest depths) of test_hip_parity._scene((H, W), 5) and 6 on a
    path of n_frames steps (test_hip_guarded.video_reference's)."""
    from ken_burns_effect_amd import common
    settings, oc = _scene((H, W), 5)
    settings = dict(settings, dblSteps=[i / (n_frames - 1) for i in range(n_frames)])
    settings.pop('boolCrop')
    cams, crop = common.frame_cameras(settings, oc), common.crop_size(settings)
    other = _scene((H, W), 6)[1]
    clouds = [[o[k].clone().contiguous() for k in ('tensorInpaPoints', 'tensorInpaImage', 'tensorInpaDepth')] for o in (oc, other)]
    near = float(min(c[0][0, 2][c[0][0, 2] > 0].min() for c in clouds))
    return cams, crop, clouds[0], clouds[1], near


def video_state(K, monkeypatch, H, W, n_frames, route, lanes):
    monkeypatch.setenv('KBE_FUSED', '1' if route == 'fused' else '0')
    monkeypatch.setenv('KBE_LANES', str(lanes))
    cams, crop, right, decoy, near = video_scene(H, W, n_frames)
    buffers = [t.clone() for t in decoy]
    state = K.prepare_cloud(*buffers, W, H, 512.0, near_depth=near)
    assert state['lanes'] == lanes and state['fused'] == (route == 'fused')
    if route == 'fused':
        return state, cams, crop, ([state['packed']], [packed_of(K, right, H, W, near)], [packed_of(K, decoy, H, W, near)])
    return state, cams, crop, (buffers, right, decoy)


VIDEO_CASES = [c.name for c in sc.cases_of('video')]


@pytest.mark.parametrize('name', VIDEO_CASES)
def test_videos_on_a_side_stream(K, monkeypatch, name):
    """kbe_render_video enqueued behind the delay.  Frames left in HBM on 1, 2 and 4 lanes, and cropped: the lanes fork from the caller's stream
    and join it again (VideoHandoff::start / join).  Delivered to pinned memory on two lanes (KBE_HOST_LANES): in groups through an SDMA engine,
    in groups through hipMemcpyAsync (KBE_HANDOFF=blit), through the staged ring and the copy stream (batch > 0, overlap), per frame by
    k_deliver (batch 0), and cropped; the host buffer starts out holding the decoy's frames, and after the side stream alone is synchronised
    it holds the right ones and the hand-off reports nothing."""
    case = sc.case('video', name)
    words = name.split()
    route = next(w for w in words if w in sc.ROUTES)
    H, W = (int(v) for v in next(w for w in words if 'x' in w and w[0].isdigit()).split('x'))
    n = dict((s[:2], s[2]) for s in sc.VIDEO_SIZES)[(H, W)]
    delivered = name.startswith('delivered')
    lanes = int(words[-1]) if 'lanes' in words else 4
    monkeypatch.setenv('KBE_HOST_LANES', '2')
    if 'hipMemcpyAsync' in name:
        monkeypatch.setenv('KBE_HANDOFF', 'blit')
    state, cams, crop, swapped = video_state(K, monkeypatch, H, W, n, route, lanes)
    out = torch.zeros(n, H, W, 3, dtype=torch.uint8, pin_memory=True) if delivered else torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')
    kw = dict(crop=crop if 'cropped' in name else None, host_out=out)
    if 'ring' in name:
        kw.update(batch=4, overlap=True)
    if 'k_deliver' in name:
        kw.update(batch=0)
    sg.hold(name, case.bar, *swapped, lambda: K.render_video(state, cams, BL, **kw), written=scratch_of(state, out), state=state)
    if delivered:
        K.handoff_status()
    if lanes > 1 or 'ring' in name:
        assert 'lane_streams' in state and sg.side_stream(state).cuda_stream not in sg.handles_in_use(state)


# ---------------------------------------------------------------------------------------
# e. the encoders and the byte-frame filters, raw
# ---------------------------------------------------------------------------------------

def photos(n, H, W, seed):
    return torch.from_numpy(np.stack([gc.photo_like(H, W, seed + i) for i in range(n)])).cuda()


def pointers(frames):
    step = frames[0].numel()
    return (ctypes.c_void_p * frames.shape[0])(*[frames.data_ptr() + i * step for i in range(frames.shape[0])])


def gif_module():
    from ken_burns_effect_amd import gif
    gif.load()
    return gif


def units_view(arrays):
    """(the buffer, the offsets, the status word) -> the same with the buffer cut at the units' end: what lies behind it is not the entry's."""
    return [arrays[0][:int(arrays[1][-1])], arrays[1], arrays[2]]


@pytest.mark.parametrize('name', ids('units'))
def test_encoders_and_filters_on_a_side_stream(K, name):
    """kbe_mjpeg_encode, kbe_png_encode and kbe_gif_encode (3 frames of 17x16; 13 of 50x37: two launches), kbe_gif_histogram (which adds to
    its counts: the zeroing is the caller's, on the same stream), kbe_gif_lut, kbe_area_reduce_u8, kbe_crop_area_u8 and kbe_dof_u8 at radius 4,
    called raw with the side stream's handle.  The buffer, the offsets, the status word and the scratch hold the decoy's bytes and get them back
    behind the delay."""
    from ken_burns_effect_amd import area, crop_area, dof
    case = sc.case('units', name)
    gif = gif_module()
    if 'frames of' in name:
        fmt, n = name.split()[0], int(name.split()[1])
        W, H = (int(v) for v in name.split()[-1].split('x'))
        right, decoy = photos(n, H, W, 3), photos(n, H, W, 40)
        frames = decoy.clone()
        lib = gif.load() if fmt == 'gif' else K.lib
        scratch = torch.zeros((int(getattr(lib, 'kbe_%s_scratch_bytes' % fmt)(W, H, n)) + 7) // 8 + 1, dtype=torch.int64, device='cuda')
        cap = n * int(getattr(lib, 'kbe_%s_bound' % fmt)(W, H))
        out, offsets, status = torch.zeros(cap, dtype=torch.uint8, device='cuda'), torch.zeros(n + 1, dtype=torch.int64, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
        table = gif.lut(gif.palette_from_histogram(gif.histogram(torch.cat([right, decoy]))))
        own = {'mjpeg': (92, 0), 'png': (0,), 'gif': (0, 8, 4, table.data_ptr())}[fmt]
        raw = gif._raw if fmt == 'gif' else K._raw

        def call():
            assert raw('kbe_%s_encode' % fmt, pointers(frames), n, W, H, 3 * W, *own, scratch.data_ptr(), out.data_ptr(), cap, offsets.data_ptr(), status.data_ptr(), stream()) == 0
            return out, offsets, status
        got, want = sg.hold(name, case.bar, [frames], [right], [decoy], call, written=lambda: [out, offsets, status, scratch], view=units_view, differ_in=[0, 1])
        assert int(want[2][0]) == 0 and int(want[1][-1]) > 0
    elif name == 'gif_histogram':
        right, decoy = (torch.from_numpy(np.stack([mc.noise(37, 50, seed + i) for i in range(13)])).cuda() for seed in (3, 40))
        frames, hist = decoy.clone(), torch.zeros(gif.CELLS, dtype=torch.int32, device='cuda')

        def call():
            hist.zero_()
            gif._call('kbe_gif_histogram', pointers(frames), 13, 50, 37, 150, 0, hist.data_ptr(), stream())
            return hist
        sg.hold(name, case.bar, [frames], [right], [decoy], call, written=lambda: [hist])
    elif name == 'gif_lut':
        rng = np.random.default_rng(5)
        right, decoy = (torch.from_numpy(rng.integers(0, 256, (256, 3), dtype=np.uint8)).cuda() for _ in range(2))
        palette, table = decoy.clone(), torch.zeros(gif.CELLS, dtype=torch.uint8, device='cuda')

        def call():
            gif._call('kbe_gif_lut', palette.data_ptr(), 256, table.data_ptr(), stream())
            return table
        sg.hold(name, case.bar, [palette], [right], [decoy], call, written=lambda: [table])
    else:
        n, H, W = 3, 37, 50
        right, decoy = photos(n, H, W, 3), photos(n, H, W, 40)
        frames = decoy.clone()
        if name == 'dof_u8 radius 4':
            z_right = torch.from_numpy(np.array(dc.depths(W, H, n), np.float32)).cuda()
            z_decoy = (z_right.flip(2) * 1.25).contiguous()
            z, out = z_decoy.clone(), torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')
            planes = (ctypes.c_void_p * n)(*[z.data_ptr() + 4 * i * H * W for i in range(n)])

            def call():
                dof._call('kbe_dof_u8', pointers(frames), planes, n, W, H, 3 * W, W, (ctypes.c_double * n)(*dc.focus_of(n)), dc.APERTURE, 4, pointers(out), 3 * W, stream())
                return out
            sg.hold(name, case.bar, [frames, z], [right, z_right], [decoy, z_decoy], call, written=lambda: [out])
        else:
            w, h = 23, 17
            out = torch.zeros(n, h, w, 3, dtype=torch.uint8, device='cuda')

            def call():
                if name == 'area_reduce_u8':
                    area._call('kbe_area_reduce_u8', pointers(frames), n, W, H, 3 * W, pointers(out), w, h, 3 * w, stream())
                else:
                    crop_area._call('kbe_crop_area_u8', pointers(frames), n, W, H, 3 * W, 45, 33, pointers(out), w, h, 3 * w, stream())
                return out
            sg.hold(name, case.bar, [frames], [right], [decoy], call, written=lambda: [out])


# ---------------------------------------------------------------------------------------
# f. the Python level, under torch.cuda.stream(s)
# ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def python_scene(K):
    """The scene of 37x50 whose cloud common.render_frames keeps resident (the fused route: the packed cloud is what is swapped), 12 cameras, its crop."""
    from ken_burns_effect_amd import common
    H, W, n = 37, 50, 12
    cams, crop, right, decoy, near = video_scene(H, W, n)
    oc = dict(_scene((H, W), 5)[1], near=near)
    oc['objectDepthrange'] = (near,) + tuple(oc['objectDepthrange'][1:])
    state = common._prepared_cloud(K, oc)
    assert state['fused'], 'KBE_FUSED is not set: the scene takes the fused route'
    return oc, state, cams, crop, ([state['packed']], [packed_of(K, right, H, W, near)], [packed_of(K, decoy, H, W, near)])


@pytest.mark.parametrize('name', ids('python')[:4])
def test_render_frames_under_a_side_stream(K, name):
    """common.render_frames inside `with torch.cuda.stream(s)`: with keep_on_device it only enqueues; delivered, reduced to an out_size and
    through a lens it synchronises s itself and returns host memory (no query() condition) -- and nothing but s."""
    from ken_burns_effect_amd import common, dof
    case = sc.case('python', name)
    oc, state, cams, crop, swapped = python_scene(K)
    H, W, n = 37, 50, len(cams)
    if name == 'render_frames keep_on_device':
        out = torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')
        call = lambda: common.render_frames(cams, oc, None, keep_on_device=True, host_out=out)
        written = scratch_of(state, out)
    else:
        kw = {'render_frames delivered': {}, 'render_frames out_size': dict(crop=crop, out_size=(20, 15)),
              'render_frames lens': dict(lens=dof.Lens(oc['near'], 2.0 * oc['near'], 20.0, 4))}[name]
        call = lambda: torch.from_numpy(common.render_frames(cams, oc, **kw).copy())
        written = scratch_of(state)
    sg.hold(name, case.bar, *swapped, call, written=written, asynchronous=case.synchronises is None, state=state)


@pytest.mark.parametrize('name', ids('python')[4:])
def test_encoding_frames_made_on_a_side_stream(K, name, tmp_path):
    """gif.write_gif and K.mjpeg_encode under the side stream on frames that the same stream has just rendered behind the delay (neither waits
    for anything but its own stream): the file and the streams are those of the same frames encoded on the default stream afterwards."""
    from ken_burns_effect_amd import common
    gif = gif_module()
    oc, state, cams, crop, (packed, packed_right, packed_decoy) = python_scene(K)
    sg.load(packed, packed_decoy)
    stale = common.render_frames(cams, oc, None, keep_on_device=True).clone()
    torch.cuda.synchronize()
    made = {}

    def call():
        frames = common.render_frames(cams, oc, None, keep_on_device=True)
        if name == 'write_gif':
            gif.write_gif(str(tmp_path / 'side.gif'), frames)
            made['units'] = (tmp_path / 'side.gif').read_bytes()
        else:
            made['units'] = b''.join(K.mjpeg_encode(frames, 92))
        return frames
    frames = sg.behind_delay(packed, packed_right, [], [], call, state=state, asynchronous=False, what=name)[0]
    if name == 'write_gif':
        gif.write_gif(str(tmp_path / 'default.gif'), frames)
        want = (tmp_path / 'default.gif').read_bytes()
    else:
        want = b''.join(K.mjpeg_encode(frames, 92))
    assert sc.differing([stale.cpu().numpy()], [frames.cpu().numpy()], 'frames')[0] >= 0.1, 'the decoy\'s frames are others'
    sg.load(packed, packed_right)
    sc.check([frames.cpu().numpy()], [common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()], 'frames', name)
    assert made['units'] == want, '%s: %d bytes for %d' % (name, len(made['units']), len(want))
