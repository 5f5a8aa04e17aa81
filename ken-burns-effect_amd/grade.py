"""Colour grading: a 3D lookup table with tetrahedral interpolation applied to frames that lie in HBM, in place (include/kbe_grade.h:
kbe_grade_u8; the arithmetic is defined in csrc/kbe_grade_block.h), and what the products need of it: the table of a .cube file (read_cube),
of simple adjustments and named looks (bake), of two tables one after the other (compose) or at another size (resample), its dwords in the
frames' channel order (quantise), and the grade of kbe.py, Pipeline and slideshow.py (grade_request, grade_for, apply_grade).

A float table is a float64 [N,N,N,3] array T with T[r, g, b] = the (R, G, B) that the colour with red r / (N - 1), green g / (N - 1) and
blue b / (N - 1) becomes, all in [0, 1] of the encoded values: nothing here is colour-managed.  The device's table is its quantised form,
N^3 dwords whose axes and bytes follow the FRAMES' channel order (quantise); the kernel knows nothing of R, G or B.

This is the only module that names the entries of kbe_grade.h: they are exported by libkbe_hip.so beside those of the other headers and
typed from their own header on the package's one handle of that library, the way the other frame filters' modules type their own.  No
fallback: without the HIP library every call here raises.
"""
import ctypes
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_grade.h')
ABI_VERSION = 1
FRAMES_PER_LAUNCH = 12             # KBE_GRADE_FRAMES_PER_LAUNCH: the entry cuts a call's frames into launches of this many
MAX_SIDE = 65535
MAX_STRENGTH = 256
MIN_NODES, MAX_NODES = 2, 33       # of the device's table, per axis
MAX_FILE_NODES = 256               # of a .cube file, which is resampled to MAX_NODES where it has more
LUMA = (0.299, 0.587, 0.114)       # Y of (R, G, B), on the encoded values
LOOKS = ('mono', 'sepia')
SEPIA_TINT = (1.00, 0.85, 0.62)    # sepia: mono, then (R, G, B) = Y * SEPIA_TINT -- black stays black, white becomes a warm cream
GRADE_KEYS = {'brightness': (0.0, 4.0), 'contrast': (0.0, 4.0), 'saturation': (0.0, 4.0), 'gamma': (0.1, 10.0)}       # --grade's keys and their ranges; every default is 1
HEADER = _cabi.Header(HEADER_PATH, 'KBE_GRADE_API', 'include/kbe_grade.h', abi=('kbe_grade_abi_version', ABI_VERSION, 'grade '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_grade.h declares, in its order, read once


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its grade entries typed from include/kbe_grade.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_grade.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


# -- the entry on tensors ------------------------------------------------------------------------
def _described(t):
    import torch
    return '%s %s on %s' % (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__


def apply(frames, table, strength=256):
    """frames: a contiguous uint8 [n,H,W,3] tensor in HBM, changed in place and returned; table: the device's table (quantise) as a
    contiguous uint8 [N,N,N,4] or int32 / uint32 [N,N,N] tensor on the same device, 2 <= N <= 33; strength: 0..256, a number, for every
    frame, or n numbers.  Asynchronous on the current stream."""
    import torch
    what = 'grade.apply'
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.size(3) == 3 and frames.size(0) >= 1 and frames.is_contiguous()):
        raise _native.KbeError('%s takes a contiguous uint8 [n,H,W,3] tensor on the GPU (frames: %s)' % (what, _described(frames)))
    words = (torch.int32,) + ((torch.uint32,) if hasattr(torch, 'uint32') else ())
    good = torch.is_tensor(table) and table.is_contiguous() and table.device == frames.device and (
        (table.dtype == torch.uint8 and table.dim() == 4 and table.size(3) == 4) or (table.dtype in words and table.dim() == 3))
    if not (good and table.size(0) == table.size(1) == table.size(2) and MIN_NODES <= table.size(0) <= MAX_NODES):
        raise _native.KbeError('%s takes a contiguous uint8 [N,N,N,4] or int32 [N,N,N] tensor on the frames\' device, %s, N = %d..%d (table: %s)' % (
            what, frames.device, MIN_NODES, MAX_NODES, _described(table)))
    n, H, W, _, pointers = _native.frame_pointers(frames, what)
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise _native.KbeError('%s: frames of %d x %d: 1..%d either way' % (what, W, H, MAX_SIDE))
    try:
        values = [strength] * n if isinstance(strength, int) and not isinstance(strength, bool) else list(strength)
        fine = len(values) == n and all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= MAX_STRENGTH for v in values)
    except TypeError:
        fine = False
    if not fine:
        raise _native.KbeError('%s: strength: a whole number or %d of them, one per frame, 0..%d' % (what, n, MAX_STRENGTH))
    _call('kbe_grade_u8', pointers, n, W, H, 3 * W, _native._ptr(table, table.dtype), int(table.size(0)), (ctypes.c_int32 * n)(*values), _native._stream())
    return frames


# -- float tables --------------------------------------------------------------------------------
def _table(table, what):
    import numpy as np
    t = np.asarray(table, dtype=np.float64)
    if not (t.ndim == 4 and t.shape[3] == 3 and t.shape[0] == t.shape[1] == t.shape[2] and t.shape[0] >= 2 and np.isfinite(t).all()):
        raise ValueError('%s takes a finite float [N,N,N,3] table, N >= 2 (got %s)' % (what, t.shape))
    return t


def grid(N):
    """The colours of the N^3 nodes: float64 [N,N,N,3], grid(N)[r, g, b] = (r, g, b) / (N - 1) -- the identity table."""
    import numpy as np
    axis = np.arange(int(N), dtype=np.float64) / (int(N) - 1)
    return np.stack(np.meshgrid(axis, axis, axis, indexing='ij'), axis=-1)


def interpolate(table, colours):
    """The float table at `colours` [..., 3] = (R, G, B), clamped to [0, 1], by the device's tetrahedral rule in float64: with x = v (N - 1),
    i = floor(x) (at most N - 2) and f = x - i per channel, the fractions ordered f_a >= f_b >= f_c, the nodes V0 = the cell's base,
    V1 = V0 + e_a, V2 = V1 + e_b, V3 = the far corner: V0 (1 - f_a) + V1 (f_a - f_b) + V2 (f_b - f_c) + V3 f_c."""
    import numpy as np
    t = _table(table, 'grade.interpolate')
    N = t.shape[0]
    x = np.clip(np.asarray(colours, dtype=np.float64), 0.0, 1.0) * (N - 1)
    i = np.minimum(np.floor(x).astype(np.int64), N - 2)
    f = x - i
    order = np.argsort(-f, axis=-1, kind='stable')
    sorted_f = np.take_along_axis(f, order, axis=-1)
    unit = np.eye(3, dtype=np.int64)
    first, second = unit[order[..., 0]], unit[order[..., 1]]
    at = [i, i + first, i + first + second, i + 1]
    weight = [1.0 - sorted_f[..., 0], sorted_f[..., 0] - sorted_f[..., 1], sorted_f[..., 1] - sorted_f[..., 2], sorted_f[..., 2]]
    return sum(w[..., None] * t[p[..., 0], p[..., 1], p[..., 2]] for w, p in zip(weight, at))


def resample(table, N):
    """The table at N nodes per axis: interpolate at the N^3 nodes' colours."""
    N = int(N)
    if N < 2:
        raise ValueError('grade.resample: N = %d: 2 or more' % N)
    return interpolate(_table(table, 'grade.resample'), grid(N))


def compose(first, then):
    """The table of `first` followed by `then`, at first's size: every node of `first`, looked up in `then` (interpolate, clamped)."""
    return interpolate(_table(then, 'grade.compose'), _table(first, 'grade.compose'))


def bake(brightness=1, contrast=1, saturation=1, gamma=1, look=None, N=33):
    """The float table [N,N,N,3] of the adjustments, on encoded values v in [0, 1], in this order: v * brightness; (v - 0.5) * contrast + 0.5;
    Y + (v - Y) * saturation with Y = 0.299 R + 0.587 G + 0.114 B (LUMA); clamp to [0, 1]; v ** (1 / gamma).  look: 'mono' is saturation 0
    whatever `saturation` says; 'sepia' is mono followed by the tint (R, G, B) = Y * SEPIA_TINT.  ValueError for a value outside GRADE_KEYS'
    ranges or an unknown look."""
    import numpy as np
    told = dict(brightness=brightness, contrast=contrast, saturation=saturation, gamma=gamma)
    for name, (low, high) in GRADE_KEYS.items():
        value = told[name]
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not low <= float(value) <= high:        # (nan fails the comparison)
            raise ValueError('grade.bake: %s = %r: %g..%g' % (name, value, low, high))
    if look is not None and look not in LOOKS:
        raise ValueError('grade.bake: look = %r: %s' % (look, ' or '.join(LOOKS)))
    if not (isinstance(N, int) and N >= 2):
        raise ValueError('grade.bake: N = %r: 2 or more' % (N,))
    v = grid(N) * float(brightness)
    v = (v - 0.5) * float(contrast) + 0.5
    Y = (v * np.asarray(LUMA)).sum(axis=-1, keepdims=True)
    v = Y + (v - Y) * (0.0 if look is not None else float(saturation))
    v = np.clip(v, 0.0, 1.0) ** (1.0 / float(gamma))
    if look == 'sepia':
        v = np.clip(v[..., :1] * np.asarray(SEPIA_TINT), 0.0, 1.0)          # (mono: the three channels are Y)
    return v


def quantise(table, bgr):
    """The device's table of a float one: clamped, round(255 x), its axes and bytes in the frames' channel order -- bgr: byte 0 of a frame's
    pixel is blue (the frames' order unless --pretrained-estim) -- and packed: uint32 [N,N,N], entry [i2, i1, i0] = the node at frame byte
    0 = i0, byte 1 = i1, byte 2 = i2, its bytes 0..2 the output's, byte 3 zero."""
    import numpy as np
    t = _table(table, 'grade.quantise')
    if not MIN_NODES <= t.shape[0] <= MAX_NODES:
        raise ValueError('grade.quantise: a table of %d nodes per axis: %d..%d (see resample)' % (t.shape[0], MIN_NODES, MAX_NODES))
    q = np.floor(255.0 * np.clip(t, 0.0, 1.0) + 0.5).astype(np.uint32)       # [r, g, b, (R, G, B)]
    if bgr:
        q = q[..., ::-1]                                                      # [i2 = r, i1 = g, i0 = b, (B, G, R)]
    else:
        q = q.transpose(2, 1, 0, 3)                                           # [i2 = b, i1 = g, i0 = r, (R, G, B)]
    return np.ascontiguousarray(q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16))


# -- .cube files -----------------------------------------------------------------------------------
def read_cube(path):
    """The table of a .cube file as a float64 [N,N,N,3] array, T[r, g, b] = (R, G, B): TITLE, comments (#) and empty lines, LUT_3D_SIZE N
    with 2 <= N <= 256, DOMAIN_MIN 0 0 0 and DOMAIN_MAX 1 1 1 (optional), then N^3 rows of three numbers, red fastest.  ValueError that names
    the file and the line for LUT_1D_SIZE, another domain, a size outside 2..256, a wrong number of rows, a malformed or non-finite number
    and anything else that is not of the format; OSError for a file that cannot be read."""
    import math
    import numpy as np

    def refuse(line, text):
        raise ValueError('%s: line %d: %s' % (path, line, text))
    N, rows, size_line, last = None, [], 0, 0
    with open(path, 'r', encoding='utf-8', errors='replace') as f:
        for number, raw in enumerate(f, 1):
            words = raw.strip().split()
            if not words or words[0].startswith('#'):
                continue
            last = number
            key = words[0]
            if key == 'TITLE':
                continue
            if key == 'LUT_1D_SIZE' or key == 'LUT_1D_INPUT_RANGE':
                refuse(number, '%s: a 1D table; only 3D tables are taken' % key)
            if key == 'LUT_3D_SIZE':
                if N is not None:
                    refuse(number, 'LUT_3D_SIZE twice')
                if len(words) != 2 or not words[1].isdigit() or not 2 <= int(words[1]) <= MAX_FILE_NODES:
                    refuse(number, 'LUT_3D_SIZE %s: a whole number 2..%d' % (' '.join(words[1:]), MAX_FILE_NODES))
                N, size_line = int(words[1]), number
                continue
            if key in ('DOMAIN_MIN', 'DOMAIN_MAX'):
                want = ['0', '0', '0'] if key == 'DOMAIN_MIN' else ['1', '1', '1']
                try:
                    same = len(words) == 4 and [float(w) for w in words[1:]] == [float(w) for w in want]
                except ValueError:
                    same = False
                if not same:
                    refuse(number, '%s %s: only the domain 0 0 0 .. 1 1 1 is taken' % (key, ' '.join(words[1:])))
                continue
            if key[0].isalpha() and key.lower() not in ('nan', 'inf', 'infinity'):
                refuse(number, 'unknown keyword %s' % key)
            if N is None:
                refuse(number, 'a row of numbers before LUT_3D_SIZE')
            try:
                values = [float(w) for w in words]
            except ValueError:
                values = []
            if len(values) != 3:
                refuse(number, 'a malformed row %r: three numbers' % raw.strip())
            if not all(math.isfinite(v) for v in values):
                refuse(number, 'a number that is not finite in %r' % raw.strip())
            if len(rows) == N ** 3:
                refuse(number, 'more than the %d rows of LUT_3D_SIZE %d' % (N ** 3, N))
            rows.append(values)
    if N is None:
        refuse(max(last, 1), 'no LUT_3D_SIZE')
    if len(rows) != N ** 3:
        refuse(max(last, size_line), '%d rows for LUT_3D_SIZE %d: %d are needed' % (len(rows), N, N ** 3))
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(N, N, N, 3).transpose(2, 1, 0, 3))      # (the file: [b][g][r])


# -- the grade of the products ---------------------------------------------------------------------
OPTIONS = ('lut', 'grade', 'look', 'lut_strength')
ENVIRONMENT = {'lut': 'KBE_LUT', 'grade': 'KBE_GRADE', 'look': 'KBE_LOOK', 'lut_strength': 'KBE_LUT_STRENGTH'}


def grade_keys(value):
    """--grade's "brightness=B,contrast=C,saturation=S,gamma=G", any subset of the keys (or a dict of them), as {key: float} within
    GRADE_KEYS' ranges, or ValueError."""
    import math
    if isinstance(value, dict):
        pairs = list(value.items())
    elif isinstance(value, str) and value.strip():
        pairs = [tuple(part.split('=', 1)) if '=' in part else (part, None) for part in value.split(',')]
    else:
        raise ValueError('%s among %s' % ('key=value pairs', ', '.join(GRADE_KEYS)))
    found = {}
    for key, text in pairs:
        key = key.strip() if isinstance(key, str) else key
        if key not in GRADE_KEYS:
            raise ValueError('unknown key %s: %s' % (key, ', '.join(GRADE_KEYS)))
        if key in found:
            raise ValueError('%s twice' % key)
        low, high = GRADE_KEYS[key]
        try:
            number = float(text) if not isinstance(text, bool) else math.nan
        except (TypeError, ValueError):
            number = math.nan
        if not low <= number <= high:
            raise ValueError('%s=%s: %g..%g' % (key, text, low, high))
        found[key] = number
    return found


def grade_request(lut=None, grade=None, look=None, lut_strength=None, environment=True):
    """What the products were told of the grade -- kbe.py's options, Pipeline's keyword arguments, else (environment) their twins KBE_LUT,
    KBE_GRADE, KBE_LOOK, KBE_LUT_STRENGTH -- read, checked and baked, on the host, before any network runs: None without a grade, else
    {'lut': path or None, 'grade': {key: value} or None, 'look', 'strength': 1..256, 'table': the finished float table -- --grade and --look
    first, then the file's table; a file of more than 33 nodes per axis resampled to 33, with a warning}.  ValueError whose text begins
    with the option at fault."""
    import math
    import warnings
    told = dict(lut=lut, grade=grade, look=look, lut_strength=lut_strength)
    if environment:
        for name, variable in ENVIRONMENT.items():
            if told[name] is None:
                told[name] = os.environ.get(variable) or None
    if told['lut'] is None and told['grade'] is None and told['look'] is None:
        if told['lut_strength'] is not None:
            raise ValueError('--lut-strength %s: only with --lut, --grade or --look' % (told['lut_strength'],))
        return None
    try:
        share = 1.0 if told['lut_strength'] is None else float(told['lut_strength'])
    except (TypeError, ValueError):
        share = 0.0
    if isinstance(told['lut_strength'], bool) or not (math.isfinite(share) and 0.0 < share <= 1.0 and int(round(MAX_STRENGTH * share)) >= 1):
        raise ValueError('--lut-strength %s: above 0 and at most 1' % (told['lut_strength'],))
    if told['look'] is not None and told['look'] not in LOOKS:
        raise ValueError('--look %s: %s' % (told['look'], ' or '.join(LOOKS)))
    keys = None
    if told['grade'] is not None:
        try:
            keys = grade_keys(told['grade'])
        except ValueError as e:
            raise ValueError('--grade %s: %s' % (told['grade'], e)) from None
    table = bake(look=told['look'], **(keys or {})) if keys is not None or told['look'] is not None else None
    if told['lut'] is not None:
        if not os.path.isfile(told['lut']):
            raise ValueError('--lut %s: no such file' % (told['lut'],))
        try:
            cube = read_cube(told['lut'])
        except (OSError, ValueError) as e:
            raise ValueError('--lut %s' % (e if str(e).startswith(str(told['lut'])) else '%s: %s' % (told['lut'], e))) from None
        if cube.shape[0] > MAX_NODES:
            warnings.warn('--lut %s: its table of %d nodes per axis is resampled to %d, the most the GPU\'s table holds' % (told['lut'], cube.shape[0], MAX_NODES))
            cube = resample(cube, MAX_NODES)
        table = cube if table is None else compose(table, cube)
    return {'lut': told['lut'], 'grade': keys, 'look': told['look'], 'strength': int(round(MAX_STRENGTH * share)), 'table': table}


def grade_for(request, bgr=True):
    """The grade of a request (grade_request) for frames in the order bgr: (the device's table as a uint32 [N,N,N] array, the strength
    1..256), or None without a request."""
    if request is None:
        return None
    return quantise(request['table'], bgr), request['strength']


def apply_grade(frames, graded):
    """grade_for's answer onto frames in HBM, every frame at its strength: in place."""
    import numpy as np
    import torch
    table, strength = graded
    return apply(frames, torch.from_numpy(np.ascontiguousarray(table).view(np.int32)).to(frames.device), strength)
