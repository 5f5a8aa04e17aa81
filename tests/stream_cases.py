"""Streams: the table of the side-stream cases (tests/test_streams_gpu.py runs them, tests/test_streams.py holds the table to the headers).

Every entry of the five headers that takes a kbe_stream_t promises to be asynchronous on THAT stream.  The rest of the GPU suite calls
everything on torch's default stream -- the null stream, on which all work serialises --, so a launch, memset or copy on stream 0, or a lane
that is not forked from and joined to the caller's stream, changes nothing it can see.  A case here makes the call on a non-blocking side stream
behind a delay, with the right inputs copied into place only behind that delay (tests/stream_gpu.py): whatever runs without a dependency
on the side stream reads the decoy that lay there before.

Importable without a GPU (NumPy only)."""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('kbe.h', 'kbe_gif.h', 'kbe_area.h', 'kbe_crop_area.h', 'kbe_dof.h')


def stream_entries(headers=HEADERS):
    """Every declaration of the headers that a KBE_*API macro marks and that has a kbe_stream_t parameter, in the headers' order."""
    found = []
    for header in headers:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', f.read(), flags=re.S)
        for name, params in re.findall(r'\bKBE_\w*API\s+[\w\s*]+?\b(\w+)\s*\(([^()]*)\)\s*;', text):
            if re.search(r'\bkbe_stream_t\b', params):
                found.append(name)
    return found


# ---------------------------------------------------------------------------------------
# the bars: none is new
# ---------------------------------------------------------------------------------------

def _as_pairs(got, want, what):
    assert len(got) == len(want), '%s: %d results for %d' % (what, len(got), len(want))
    return list(zip(got, want))


def _check_bits(got, want, what):
    for i, (a, b) in enumerate(_as_pairs(got, want, what)):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), '%s: result %d differs from the default stream\'s in %d of %d elements' % (
            what, i, int((a != b).sum()) if a.shape == b.shape else -1, b.size)


def _check_atomic(got, want, what):
    for i, (a, b) in enumerate(_as_pairs(got, want, what)):
        assert a.shape == b.shape and np.array_equal(a == 0, b == 0), '%s: result %d: the same pixels and channels are touched' % (what, i)
        assert (np.abs(a - b) <= 2e-5 * np.maximum(np.abs(b), 1.0)).all(), '%s: result %d' % (what, i)


def _frames(bound):
    def check(got, want, what):
        for i, (a, b) in enumerate(_as_pairs(got, want, what)):
            assert a.shape == b.shape, (what, a.shape, b.shape)
            d = np.abs(a.astype(np.int32) - b.astype(np.int32))
            assert d.max() <= bound and (d > 0).mean() < 1e-3 and (d > 1).mean() < 1e-5, '%s: result %d: max %d, %.2e of the values differ, %.2e by more than one' % (
                what, i, d.max(), (d > 0).mean(), (d > 1).mean())
    return check


# check(got, want, what): raises unless the lists of arrays agree under the bar; beyond(a, b): the elements of two arrays that are further apart
# than the bar allows two right results to be (what a decoy has to be in a tenth of its elements)
Bar = collections.namedtuple('Bar', 'text check beyond')
BARS = {
    'bits': Bar('bit for bit', _check_bits, lambda a, b: a != b),
    'atomic': Bar('the same pixels touched, 2e-5 relative (test_glue_and_network_kernels_write_only_their_outputs)', _check_atomic,
                  lambda a, b: np.abs(a - b) > 2e-5 * np.maximum(np.abs(b), 1.0)),
    'frames': Bar('<= 1 count on < 0.1 % of the values (DESIGN section 2)', _frames(1), lambda a, b: np.abs(a.astype(np.int32) - b.astype(np.int32)) > 1),
    'cropped frames': Bar('<= 1 count on < 0.1 % of the values, <= 2 through the crop\'s fixed point on < 1e-5 (DESIGN section 2)', _frames(2),
                          lambda a, b: np.abs(a.astype(np.int32) - b.astype(np.int32)) > 2),
}


def bars_of(bar, n):
    """A case's bar for each of its n results: one name for all, or one per result joined by ' / '."""
    names = bar.split(' / ')
    assert len(names) in (1, n), (bar, n)
    return names * n if len(names) == 1 else names


def differing(a, b, bar):
    """The share of the elements of two lists of arrays that lie further apart than the bar allows, per pair (results of two lengths -- the
    bytes of two sets of units --: over the longer one, what the shorter one lacks counted as different)."""
    shares = []
    for x, y, name in zip(a, b, bars_of(bar, len(a))):
        m = min(x.size, y.size)
        if x.shape != y.shape:
            x, y = x.reshape(-1)[:m], y.reshape(-1)[:m]
        longer = max(a[len(shares)].size, b[len(shares)].size)
        shares.append((float(np.sum(BARS[name].beyond(x, y))) + longer - m) / longer if longer else 0.0)
    return shares


def check(got, want, bar, what):
    """Raises unless every result agrees with the right one under its bar."""
    assert len(got) == len(want), '%s: %d results for %d' % (what, len(got), len(want))
    for i, name in enumerate(bars_of(bar, len(want))):
        BARS[name].check(got[i:i + 1], want[i:i + 1], '%s, result %d' % (what, i))


# ---------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------

# group: the part of tests/test_streams_gpu.py that runs the case; entries: the declarations with a kbe_stream_t the case calls on the side stream;
# bar: a key of BARS; synchronises: None, or why the tensor-level call synchronises the stream by contract (then no query() condition)
Case = collections.namedtuple('Case', 'group name entries bar synchronises')

# (a) test_hip_guarded.glue_calls' thunks by name -> (entries, bar)
GLUE = {
    'depth_to_points': (('kbe_depth_to_points',), 'bits'),
    'depth_to_points valid': (('kbe_depth_to_points',), 'bits'),
    'shift_points': (('kbe_shift_points',), 'bits'),
    'laplacian': (('kbe_spatial_filter',), 'bits'),
    'median-3': (('kbe_spatial_filter',), 'bits'),
    'median-5': (('kbe_spatial_filter',), 'bits'),
    'laplacian_valid': (('kbe_laplacian_valid',), 'bits'),
    'zsplat': (('kbe_zkeys_clear', 'kbe_zsplat'), 'bits'),
    'zkeys_decode': (('kbe_zkeys_decode',), 'bits'),
    'degrid': (('kbe_degrid',), 'bits'),
    'degrid from fp32': (('kbe_zkeys_decode', 'kbe_degrid'), 'bits'),
    'degrid_serial': (('kbe_degrid_serial',), 'bits'),
    'accumulate': (('kbe_accumulate',), 'atomic'),
    'normalize': (('kbe_normalize',), 'bits'),
    'render_pointcloud atomic C=4': (('kbe_render_pointcloud',), 'atomic'),
    'render_pointcloud atomic C=7': (('kbe_render_pointcloud',), 'atomic'),
    'render_pointcloud tiled C=4': (('kbe_render_pointcloud_tiled',), 'atomic'),
    'render_pointcloud tiled C=7': (('kbe_render_pointcloud_tiled',), 'atomic'),
    'fill_disocclusion': (('kbe_fill_disocclusion',), 'bits'),
    'generate_mask tables': (('kbe_generate_mask',), 'bits'),
    'generate_mask': (('kbe_generate_mask', 'kbe_spatial_filter'), 'bits'),
    'frame_u8': (('kbe_frame_u8',), 'bits'),
    'crop_resize_u8': (('kbe_crop_resize_u8',), 'bits'),
    'pconv_epilogue': (('kbe_pconv_epilogue',), 'bits'),
    'pconv_epilogue slope residual': (('kbe_pconv_epilogue',), 'bits'),
    'pconv_epilogue raw_without_bias': (('kbe_pconv_epilogue',), 'bits'),
    'pconv_epilogue no mask': (('kbe_pconv_epilogue',), 'bits'),
    'prelu_mask': (('kbe_prelu_mask',), 'bits'),
    'prelu_mask no mask': (('kbe_prelu_mask',), 'bits'),
    'bias_act': (('kbe_bias_act',), 'bits'),
    'bias_act bare': (('kbe_bias_act',), 'bits'),
    'upsample2x_act': (('kbe_upsample2x_act',), 'bits'),
    'upsample2x_act bare': (('kbe_upsample2x_act',), 'bits'),
    # (not of glue_calls: the two self-tests have wrappers and a stream like the rest)
    'selftest_err': (('kbe_selftest_err',), 'bits'),
    'selftest_division': (('kbe_selftest_division',), 'bits'),
}
GLUE_SHAPE = (2, 3, 7, 9)
VECTOR_SHAPE = (1, 5, 12, 20)           # HW % 4 == 0 and 16-byte aligned operands: k_bias_act<true>
VECTOR_THUNKS = ('bias_act', 'bias_act bare')

RASTERS = ((37, 50), (32, 64))
VIDEO_SIZES = ((37, 50, 12), (64, 96, 16))           # (H, W, frames)
ROUTES = ('fused', 'bucket')
ENCODER_SHAPES = ((3, 16, 17), (13, 37, 50))         # (frames, H, W): 3 frames of 17x16, 13 of 50x37 -- the second takes two launches

# one frame with every optional output: the frame; the z-buffer before and after degrid (bit-exact); the accumulated weight and the
# filled float render (summed in the order the records reach a tile: the float bound)
ONE_FRAME = 'frames / bits / bits / atomic / atomic'
UNITS = 'bits / bits / bits'       # the units' bytes, the offsets, the status word
SYNC_UNITS = 'encode_units reads the offsets and the status word back (meta.cpu())'
SYNC_DELIVERED = 'render_frames without keep_on_device synchronises the stream and returns host memory'


def _cases():
    rows = [Case('glue', name, entries, bar, None) for name, (entries, bar) in GLUE.items()]
    rows += [Case('abi', 'render_pointcloud', ('kbe_render_pointcloud',), 'atomic', None),
             Case('abi', 'degrid_serial from fp32', ('kbe_degrid_serial',), 'bits', None),
             Case('abi', 'zkeys_clear', ('kbe_zkeys_clear',), 'bits', None)]
    for H, W in RASTERS:
        size = '%dx%d' % (H, W)
        rows += [Case('frame', 'scratch_init %s' % size, ('kbe_frame_scratch_init', 'kbe_render_frame'), 'frames', None),
                 Case('frame', 'scratch_init_sets %s' % size, ('kbe_frame_scratch_init_sets', 'kbe_render_frame_stages'), 'frames', None),
                 Case('frame', 'cloud_pack %s' % size, ('kbe_cloud_pack', 'kbe_render_frame_fused'), 'frames', None),
                 Case('frame', 'one frame fused %s' % size, ('kbe_render_frame_fused',), ONE_FRAME, None),
                 Case('frame', 'one frame bucket %s' % size, ('kbe_render_frame_stages',), ONE_FRAME, None),
                 Case('frame', 'one frame generic %s' % size, ('kbe_shift_points', 'kbe_render_pointcloud', 'kbe_fill_disocclusion', 'kbe_frame_u8'), 'frames', None),
                 Case('frame', 'group %s' % size, ('kbe_render_frame_group',), 'frames', None),
                 Case('frame', 'group_fused %s' % size, ('kbe_render_frame_group_fused',), 'frames', None),
                 Case('frame', 'group_ahead %s' % size, ('kbe_render_frame_group_ahead',), 'frames', None),
                 Case('frame', 'render_pointcloud_tiled %s' % size, ('kbe_render_pointcloud_tiled',), 'atomic', None)]
    for H, W, n in VIDEO_SIZES:
        for route in ROUTES:
            where = '%dx%d %s' % (H, W, route)
            rows += [Case('video', 'in HBM %s lanes %d' % (where, lanes), ('kbe_render_video',), 'frames', None) for lanes in (1, 2, 4)]
            rows += [Case('video', 'in HBM cropped %s' % where, ('kbe_render_video',), 'cropped frames', None),
                     Case('video', 'delivered by SDMA %s' % where, ('kbe_render_video',), 'frames', None),
                     Case('video', 'delivered by hipMemcpyAsync %s' % where, ('kbe_render_video',), 'frames', None),
                     Case('video', 'delivered by the ring %s' % where, ('kbe_render_video',), 'frames', None),
                     Case('video', 'delivered by k_deliver %s' % where, ('kbe_render_video',), 'frames', None),
                     Case('video', 'delivered cropped %s' % where, ('kbe_render_video',), 'cropped frames', None)]
    for n, H, W in ENCODER_SHAPES:
        rows += [Case('units', '%s %d frames of %dx%d' % (fmt, n, W, H), ('kbe_%s_encode' % fmt,), UNITS, None) for fmt in ('mjpeg', 'png', 'gif')]
    rows += [Case('units', 'gif_histogram', ('kbe_gif_histogram',), 'bits', None),
             Case('units', 'gif_lut', ('kbe_gif_lut',), 'bits', None),
             Case('units', 'area_reduce_u8', ('kbe_area_reduce_u8',), 'bits', None),
             Case('units', 'crop_area_u8', ('kbe_crop_area_u8',), 'bits', None),
             Case('units', 'dof_u8 radius 4', ('kbe_dof_u8',), 'bits', None)]
    rows += [Case('python', 'render_frames keep_on_device', ('kbe_render_video',), 'frames', None),
             Case('python', 'render_frames delivered', ('kbe_render_video',), 'frames', SYNC_DELIVERED),
             Case('python', 'render_frames out_size', ('kbe_render_video', 'kbe_crop_area_u8'), 'frames', SYNC_DELIVERED),
             Case('python', 'render_frames lens', ('kbe_render_frame_fused', 'kbe_dof_u8'), 'frames', SYNC_DELIVERED),
             Case('python', 'write_gif', ('kbe_gif_histogram', 'kbe_gif_lut', 'kbe_gif_encode'), 'bits', SYNC_UNITS),
             Case('python', 'mjpeg_encode', ('kbe_mjpeg_encode',), 'bits', SYNC_UNITS)]
    return rows


CASES = _cases()


def cases_of(group):
    return [c for c in CASES if c.group == group]


def case(group, name):
    found = [c for c in CASES if c.group == group and c.name == name]
    assert len(found) == 1, (group, name)
    return found[0]
