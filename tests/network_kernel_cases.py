"""The cases and the references of tests/test_network_kernels_gpu.py: the four element-wise kernels the networks run between their
convolutions (csrc/kbe_hip.hip: kbe_pconv_epilogue, kbe_prelu_mask, kbe_bias_act, kbe_upsample2x_act).  Nothing here needs a GPU;
tests/test_network_kernel_cases.py pins the references to what the suite already trusts.

References.  pconv_epilogue, prelu_mask and bias_act are restated in NumPy float32, ONE IEEE operation at a time, in the order include/kbe.h
states: the library is built with -ffp-contract=off and its division is the correctly rounded one, so the contract is bits (an expected NaN
asks for a NaN, whatever its payload).  upsample2x_act is held to the float64 value of its own definition under a bound per output element.

Every array a function here returns is freshly made or read-only: the tests share them and leave them unchanged.
"""
import collections
import functools
import itertools

import numpy as np

F32 = np.float32
U = 2.0 ** -24                              # the unit roundoff of fp32
FLT_MAX = np.finfo(np.float32).max
SUB_MIN = np.uint32(0x00000001).view(np.float32)        # the smallest subnormal
SUB_MAX = np.uint32(0x007FFFFF).view(np.float32)        # the largest
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, FLT_MAX, -FLT_MAX], dtype=np.float32)


def _quiet(fn):
    """inf - inf, 0 * inf and overflow are part of the cases: no warnings"""
    @functools.wraps(fn)
    def run(*args, **kwargs):
        with np.errstate(all='ignore'):
            return fn(*args, **kwargs)
    return run


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def is_subnormal(a):
    a = np.asarray(a, dtype=np.float32)
    return (a != 0) & (np.abs(a) < np.finfo(np.float32).tiny)


def same_bits(got, want):
    """Elementwise: the same bit pattern, or a NaN where a NaN is expected."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return (np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def assert_same_bits(got, want, what):
    ok = same_bits(got, want)
    if not ok.all():
        at = tuple(int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError('%s: %d of %d elements differ in their bits, the first at %s: got %r (0x%08x), want %r (0x%08x)'
                             % (what, (~ok).sum(), ok.size, at, float(np.asarray(got)[at]), int(np.asarray(got, dtype=np.float32)[at].view(np.uint32)),
                                float(np.asarray(want)[at]), int(np.asarray(want, dtype=np.float32)[at].view(np.uint32))))


def scatter_specials(a, seed, values=SPECIALS):
    """`a` with the special values, the list over and over, at every eighth element or so -> (the array, the bool mask of where they went).
    Arrays smaller than the list take its head, rotated by the seed."""
    a = np.array(a, dtype=np.float32)
    flat = a.reshape(-1)
    n = flat.size
    values = np.roll(values, -seed)
    count = max(min(n, len(values)), n // 8)
    step = max(1, n // count)
    where = (np.arange(count) * step + (seed * 7) % step) % n
    flat[where] = np.resize(values, count)
    put = np.zeros(n, bool)
    put[where] = True
    return a, put.reshape(a.shape)


@_quiet
def prelu(v, slope):
    """torch.nn.functional.prelu, to the sign of a zero: v > 0 ? v : slope * v (a NaN takes the product).  slope broadcasts."""
    return np.where(v > 0, v, (slope * v).astype(v.dtype))


def _per_channel(vec, dtype):
    return np.asarray(vec, dtype=np.float32).astype(dtype).reshape(1, -1, 1, 1)


def slopes(C, start=0):
    """C slopes, every one different: 0, 1, a negative one and 0.25 first (rotated by `start`), then values of no pattern."""
    base = [0.0, 1.0, -0.5, 0.25]
    base = base[start % 4:] + base[:start % 4]
    more = [0.03125 * (j + 1) * (-1) ** j + 0.011 * j for j in range(max(0, C - 4))]
    out = np.array((base + more)[:C], dtype=np.float32)
    assert len(set(out.tolist())) == C
    return out


# ---------------------------------------------------------------------------------------
# kbe_pconv_epilogue
# ---------------------------------------------------------------------------------------

GEOMETRIES = [(1, 1, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0), (3, 1, 3), (2, 2, 0), (4, 2, 1), (5, 1, 2), (5, 2, 2), (7, 2, 3)]       # (k, stride, pad)
GOLDEN_GEOMETRIES = {(3, 1, 1): 'a', (3, 2, 1): 'b', (1, 1, 0): 'c'}        # tests/golden/partial_conv.npz: cfg_*, at 10 x 12 with B = 2
EVERYWHERE = [(17, 23), (1, 1), (5, 300)]                                   # inputs (H, W) every geometry runs on, where they leave an output
ONLY_AT = {(3, 1, 1): [(16, 16)], (1, 1, 0): [(1, 257)]}                    # Ho Wo = 256: exactly one block; 257: one thread in the second
MASK_FORMS = ['per channel', 'one channel', 'none', 'ones', 'zeros']
# (bias, raw_without_bias, act_slope, residual): raw_without_bias without a bias is the plain call, which the wrapper folds
OPERANDS = [(b, w, s, r) for b, w, s, r in itertools.product((True, False), (True, False), (True, False), (True, False)) if b or not w]
FULL = (True, True, True, True)

PconvCase = collections.namedtuple('PconvCase', 'name k stride pad B Cin Cout H W Ho Wo form operands seed')


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


@functools.lru_cache(maxsize=None)
def pconv_cases():
    """Every (geometry, mask form) pair with the full operand set on 17 x 23, the other inputs rotating through the operand combinations, B in
    {1, 3}, Cin in {1, 3, 5} and Cout in {1, 4} rotating with them."""
    cases, turn = [], 0
    for (k, stride, pad) in GEOMETRIES:
        for (H, W) in EVERYWHERE + ONLY_AT.get((k, stride, pad), []):
            Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
            if Ho < 1 or Wo < 1:
                continue
            for form in MASK_FORMS:
                operands = FULL if (H, W) == (17, 23) else OPERANDS[turn % len(OPERANDS)]
                B, Cin, Cout = (1, 3)[turn % 2], (1, 3, 5)[turn % 3], (1, 4)[(turn // 2) % 2]
                if form == 'one channel' and Cin == 1:
                    Cin = (3, 5)[turn % 2]                  # the one-channel mask of a layer with several input channels
                name = 'k%d s%d p%d %dx%d %s B%d Cin%d Cout%d %s' % (k, stride, pad, H, W, form, B, Cin, Cout, ''.join('01'[v] for v in operands))
                cases.append(PconvCase(name, k, stride, pad, B, Cin, Cout, H, W, Ho, Wo, form, operands, 1000 + turn))
                turn += 1
    return tuple(cases)


def pconv_mask(cs, rng):
    """The mask the entry is given (None for 'none'): 0/1 with one rectangle of zeros larger than the kernel, on every channel."""
    if cs.form == 'none':
        return None
    Cm = 1 if cs.form == 'one channel' else cs.Cin
    if cs.form == 'ones':
        return np.ones((cs.B, Cm, cs.H, cs.W), np.float32)
    if cs.form == 'zeros':
        return np.zeros((cs.B, Cm, cs.H, cs.W), np.float32)
    m = (rng.random((cs.B, Cm, cs.H, cs.W)) < 0.7).astype(np.float32)
    side = cs.k + 2
    for b in range(cs.B):
        y0, x0 = int(rng.integers(0, max(1, cs.H - side + 1))), int(rng.integers(0, max(1, cs.W - side + 1)))
        m[b, :, y0:y0 + side, x0:x0 + side] = 0.0
    return m


@functools.lru_cache(maxsize=None)
def pconv_inputs(cs):
    """dict(raw, bias, mask, slope, residual) of a case, each None where the case does not pass it; read-only."""
    rng = np.random.default_rng(cs.seed)
    use_bias, _, use_slope, use_res = cs.operands
    shape = (cs.B, cs.Cout, cs.Ho, cs.Wo)
    mask = pconv_mask(cs, rng)
    return {'raw': frozen(rng.standard_normal(shape).astype(np.float32)),
            'bias': frozen(rng.standard_normal(cs.Cout).astype(np.float32)) if use_bias else None,
            'mask': None if mask is None else frozen(mask),
            'slope': frozen(slopes(cs.Cout, cs.seed)) if use_slope else None,
            'residual': frozen(rng.standard_normal(shape).astype(np.float32)) if use_res else None}


def pconv_kwargs(cs):
    """What the wrapper (K.pconv_epilogue / oracle.pconv_epilogue) gets besides raw, bias, mask, k, stride, pad."""
    return {'in_channels': cs.Cin, 'in_size': (cs.H, cs.W)}


def window_sums(B, mask, k, stride, pad, in_channels=None, in_size=None, dtype=np.float32):
    """(msum [B,Ho,Wo], Cin): the mask summed over every window's Cin k k taps, one addition at a time in the kernel's loop order (channel,
    ky, kx); a tap in the padding adds nothing (the kernel skips it: x + 0 is x).  A one-channel mask of Cin channels: Cin times its sum."""
    if mask is not None:
        _, Cm, H, W = mask.shape
        Cin = Cm if in_channels is None else int(in_channels)
        planes = np.asarray(mask, dtype=np.float32).astype(dtype)
    else:
        Cin, (H, W) = int(in_channels), in_size
        planes = np.ones((B, 1, H, W), dtype)
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    padded = np.zeros((B, planes.shape[1], H + 2 * pad + stride, W + 2 * pad + stride), dtype)
    padded[:, :, pad:pad + H, pad:pad + W] = planes
    msum = np.zeros((B, Ho, Wo), dtype)
    for ci in range(planes.shape[1]):
        for ky in range(k):
            for kx in range(k):
                msum = msum + padded[:, ci, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
    if planes.shape[1] != Cin:
        msum = dtype(Cin) * msum
    return msum, Cin


@_quiet
def pconv_reference(raw, bias, mask, k, stride, pad, in_channels=None, in_size=None, act_slope=None, residual=None, raw_without_bias=False,
                    dtype=np.float32):
    """include/kbe.h, kbe_pconv_epilogue, one operation at a time in `dtype` -> (out [B,Cout,Ho,Wo], um [B,1,Ho,Wo]).  The window sum runs in
    the kernel's loop order (channel, ky, kx); a tap in the padding adds nothing (the kernel skips it: x + 0 is x)."""
    B, Cout, Ho, Wo = raw.shape
    msum, Cin = window_sums(B, mask, k, stride, pad, in_channels, in_size, dtype)
    assert msum.shape == (B, Ho, Wo)
    ratio = dtype(Cin * k * k) / (msum + dtype(np.float32(1e-8)))
    um = np.where(msum < 0, dtype(0), np.where(msum > 1, dtype(1), msum)).astype(dtype)
    ratio = (ratio * um)[:, None]
    r = np.asarray(raw, dtype=np.float32).astype(dtype)
    if bias is not None:
        bv = _per_channel(bias, dtype)
        rb = r + bv if raw_without_bias else r
        v = (((rb - bv) * ratio) + bv) * um[:, None]
    else:
        v = r * ratio
    if residual is not None:
        v = v + np.asarray(residual, dtype=np.float32).astype(dtype)
    if act_slope is not None:
        v = prelu(v, _per_channel(act_slope, dtype))
    return v.astype(dtype), um[:, None].astype(dtype)


def pconv_expected(cs, inputs=None):
    """(out, um) of a case in fp32.  A one-channel mask is held to the bits of the same mask on every one of the Cin channels."""
    x = pconv_inputs(cs) if inputs is None else inputs
    mask = x['mask']
    if mask is not None and mask.shape[1] == 1 and cs.Cin > 1:
        mask = np.repeat(mask, cs.Cin, axis=1)
    return pconv_reference(x['raw'], x['bias'], mask, cs.k, cs.stride, cs.pad, cs.Cin, (cs.H, cs.W), x['slope'], x['residual'], cs.operands[1])


# -- special values in raw and residual --

SPECIAL_PCONV = [cs for cs in pconv_cases() if (cs.H, cs.W) == (17, 23) and cs.form in ('per channel', 'none') and (cs.k, cs.stride, cs.pad) in ((3, 1, 1), (3, 1, 3), (4, 2, 1), (7, 2, 3))]


def pconv_special_inputs(cs):
    """The case's inputs with the special values scattered over raw and (elsewhere) over residual, and raw elements equal to their channel's
    bias and to its negative (rb - bv = +0; with raw_without_bias r + bv = +0) -> (inputs, touched [B,Cout,Ho,Wo]: the elements that hold one)."""
    x = dict(pconv_inputs(cs))
    raw, at_raw = scatter_specials(x['raw'], cs.seed)
    res, at_res = scatter_specials(x['residual'], cs.seed + 5)
    touched = at_raw | at_res
    n = cs.Ho * cs.Wo
    for b in range(cs.B):
        for co in range(cs.Cout):
            for j, value in enumerate((x['bias'][co], -x['bias'][co])):
                i = (31 * co + 17 * b + 5 + 3 * j) % n
                if not touched[b, co].reshape(-1)[i]:
                    raw[b, co].reshape(-1)[i] = value
                    touched[b, co].reshape(-1)[i] = True
    x['raw'], x['residual'] = frozen(raw), frozen(res)
    return x, touched


# -- fractional masks --

FRACTIONAL_PCONV = [PconvCase('fractional k3 s1 p1 17x23', 3, 1, 1, 3, 5, 4, 17, 23, 17, 23, 'fractional', (True, False, False, False), 77),
                    PconvCase('fractional k5 s2 p2 17x23', 5, 2, 2, 1, 3, 4, 17, 23, 9, 12, 'fractional', (False, False, False, False), 78),
                    PconvCase('fractional k5 s2 p2 17x23 bias', 5, 2, 2, 1, 3, 4, 17, 23, 9, 12, 'fractional', (True, False, False, False), 79)]


@functools.lru_cache(maxsize=None)
def fractional_inputs(cs):
    rng = np.random.default_rng(cs.seed)
    shape = (cs.B, cs.Cout, cs.Ho, cs.Wo)
    mask = rng.random((cs.B, cs.Cin, cs.H, cs.W)).astype(np.float32)
    # fading in from the left, by 1.3 a column: window sums below 1 (um = msum, not the clamp's 1), between 1 and 2, and above
    mask *= np.minimum(1.0, 0.004 * 1.3 ** np.arange(cs.W)).astype(np.float32)
    return {'raw': frozen(rng.standard_normal(shape).astype(np.float32)), 'bias': frozen(rng.standard_normal(cs.Cout).astype(np.float32)) if cs.operands[0] else None,
            'mask': frozen(mask), 'slope': None, 'residual': None}


@_quiet
def fractional_bounds(cs):
    """(out64, um64, the bound on |out - out64|, the bound on |um - um64|) of a fractional-mask case, every array float64.

    The order in which a convolution with ones sums its n = Cin k k taps is nobody's contract, so the fp32 result is held to the exact value
    (float64 here: its own error is 2^-29 of the bounds below) under the bound any order of summation keeps.  With u = 2^-24 and all taps >= 0,
    recursive summation in any order gives msum' = msum (1 + a), |a| <= g = (n - 1) u / (1 - (n - 1) u) [Higham, Accuracy and Stability of
    Numerical Algorithms, (4.4)].  The five operations that follow, each rounding once (|b..e| <= u), and the clamp, which rounds nothing:
        s'  = (msum' + 1e-8f)(1 + b)          1e-8f is exact and of msum's sign: s' = s (1 + a1)(1 + b), |a1| <= g
        q'  = N / s' (1 + c)                  N = Cin k k is exact:              q' = q (1 + c) / ((1 + a1)(1 + b))
        um' = clamp(msum', 0, 1)              monotone, 1-Lipschitz, um <= msum: um' = um (1 + a2), |a2| <= g   <- the bound on um: g um
        r'  = q' um' (1 + d)                  r' = r (1 + E),  1 + E <= (1 + u)^2 (1 + g) / ((1 - g)(1 - u)) =: 1 + Er
        out' = raw r' (1 + e)                 (no bias)  |out' - out| <= |out| ((1 + Er)(1 + u) - 1)
    and with a bias, out = ((raw - bias) r + bias) um:
        t1' = (raw - bias)(1 + e1);  t2' = t1' r' (1 + e2):  |t2' - t2| <= |t2| E2,  1 + E2 = (1 + Er)(1 + u)^2
        t3' = (t2' + bias)(1 + e3):                          |t3' - t3| <= err3 = |t2| E2 + u (|t3| + |t2| E2)
        out' = t3' um' (1 + e4):                             |out' - out| <= um ((|t3| + err3)(1 + g)(1 + u) - |t3|)
    To first order that is (2 (n - 1) + 4) u |out| without a bias: 92 u at Cin k k = 45, 152 u at 75."""
    x = fractional_inputs(cs)
    out64, um64 = pconv_reference(x['raw'], x['bias'], x['mask'], cs.k, cs.stride, cs.pad, cs.Cin, (cs.H, cs.W), dtype=np.float64)
    n = cs.Cin * cs.k * cs.k
    g = (n - 1) * U / (1 - (n - 1) * U)
    Er = (1 + U) ** 2 * (1 + g) / ((1 - g) * (1 - U)) - 1
    if x['bias'] is None:
        out_bound = np.abs(out64) * ((1 + Er) * (1 + U) - 1)
    else:
        # r from the same float64 evaluation: without a bias a raw of 1 comes out as r
        r, _ = pconv_reference(np.ones_like(x['raw']), None, x['mask'], cs.k, cs.stride, cs.pad, cs.Cin, (cs.H, cs.W), dtype=np.float64)
        bias = _per_channel(x['bias'], np.float64)
        t2 = (x['raw'].astype(np.float64) - bias) * r
        t2, t3 = np.abs(t2), np.abs(t2 + bias)
        E2 = (1 + Er) * (1 + U) ** 2 - 1
        err3 = t2 * E2 + U * (t3 + t2 * E2)
        out_bound = um64 * ((t3 + err3) * (1 + g) * (1 + U) - t3)
    return out64, um64, out_bound, g * um64


# ---------------------------------------------------------------------------------------
# kbe_prelu_mask, kbe_bias_act, kbe_upsample2x_act
# ---------------------------------------------------------------------------------------

SHAPES = [(1, 1, 1, 1), (2, 3, 7, 9), (1, 5, 16, 16), (1, 2, 1, 257), (3, 4, 17, 23), (1, 64, 4, 4)]      # (B, C, H, W)
BIAS_ACT_SHAPES = SHAPES + [(1, 3, 32, 32), (1, 3, 32, 33)]       # HW / 4 = 256 and 264 on the vector path: one block, and a second
UPSAMPLE_SHAPES = SHAPES + [(1, 3, 5, 1), (1, 2, 3, 255), (1, 2, 2, 256), (2, 2, 3, 257), (1, 3, 33, 47)]
PRELU_MASK_FORMS = ['01', 'fractional', 'none']
ALIGNMENT_SHAPE = (2, 3, 8, 12)             # HW % 4 == 0: the vector path when every pointer is 16-byte aligned, else the scalar one
ORDER_SHAPES = [(1, 3, 32, 32), (2, 3, 7, 9)]


def _seed_of(shape, salt=0):
    B, C, H, W = shape
    return ((B * 131 + C) * 131 + H) * 131 + W + 7919 * salt


@functools.lru_cache(maxsize=None)
def prelu_mask_inputs(shape, form):
    """dict(x, slope, mask): the special values in x, and under a mask a 0 over +inf and over -inf (torch.mul gives NaN there)."""
    B, C, H, W = shape
    rng = np.random.default_rng(_seed_of(shape, 1))
    x, put = scatter_specials(rng.standard_normal(shape), _seed_of(shape))
    mask = None
    if form != 'none':
        mask = (rng.random((B, 1, H, W)) < 0.6).astype(np.float32) if form == '01' else rng.random((B, 1, H, W)).astype(np.float32)
        infinite = np.isinf(x).any(axis=1, keepdims=True)
        mask[infinite] = 0.0
    return {'x': frozen(x), 'slope': frozen(slopes(C, B + C + W)), 'mask': None if mask is None else frozen(mask)}


@_quiet
def prelu_mask_reference(x, slope, mask):
    v = prelu(np.asarray(x, dtype=np.float32), _per_channel(slope, np.float32))
    return v if mask is None else (v * np.asarray(mask, dtype=np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def bias_act_inputs(shape):
    """dict(x, bias, slope, res1, res2): the special values in x, res1 and res2; per plane an x that cancels its bias to +0 (a negative slope
    then gives -0); where C > 1 the last channel's bias is 3e38 and one of its elements FLT_MAX, so that x + bias overflows to inf."""
    B, C, H, W = shape
    rng = np.random.default_rng(_seed_of(shape, 2))
    seed = _seed_of(shape)
    x, _ = scatter_specials(rng.standard_normal(shape), seed)
    res1, _ = scatter_specials(rng.standard_normal(shape), seed + 3)
    res2, _ = scatter_specials(rng.standard_normal(shape), seed + 6)
    bias = rng.standard_normal(C).astype(np.float32)
    if C > 1:
        bias[C - 1] = np.float32(3e38)
    flat = x.reshape(B, C, H * W)
    for b in range(B):
        for c in range(C):
            i = (7 * c + 3 * b + 1) % (H * W)
            flat[b, c, i] = -bias[c]
            j = (i + 2) % (H * W)
            if c == C - 1 and C > 1 and j != i:
                flat[b, c, j] = FLT_MAX
    return {'x': frozen(x), 'bias': frozen(bias), 'slope': frozen(slopes(C, B + C + W)), 'res1': frozen(res1), 'res2': frozen(res2)}


BIAS_ACT_OPERANDS = list(itertools.product((False, True), (False, True), (0, 1, 2)))        # (bias, slope, residuals)


@_quiet
def bias_act_reference(x, bias=None, slope=None, res1=None, res2=None, swap_residuals=False):
    """(act(x + bias[c]) + res1) + res2, each step one fp32 operation.  swap_residuals: the other order, (act(..) + res2) + res1."""
    v = np.asarray(x, dtype=np.float32)
    if bias is not None:
        v = v + _per_channel(bias, np.float32)
    if slope is not None:
        v = prelu(v, _per_channel(slope, np.float32))
    for r in ((res2, res1) if swap_residuals else (res1, res2)):
        if r is not None:
            v = v + np.asarray(r, dtype=np.float32)
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def order_inputs(shape):
    """Values of order 1 to 10 under an r1 of 1e8 to 2e8 (spacing 8 or 16) and an r2 of their own order: (v + r1) + r2 rounds v and r2 to the
    spacing one after the other, (v + r2) + r1 rounds their sum -- another multiple wherever the two roundings do not add up.  (An r2 of -r1
    would not do: both orders then round v alone.)"""
    B, C, H, W = shape
    rng = np.random.default_rng(_seed_of(shape, 3))
    x = (rng.standard_normal(shape) * 6).astype(np.float32)
    r1 = (np.float32(1e8) * (1 + rng.random(shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    r2 = (rng.standard_normal(shape) * 6).astype(np.float32)
    return {'x': frozen(x), 'bias': frozen(rng.standard_normal(C).astype(np.float32)), 'slope': frozen(slopes(C, 1)), 'res1': frozen(r1), 'res2': frozen(r2)}


# -- upsample --

@functools.lru_cache(maxsize=None)
def upsample_inputs(shape):
    """x with magnitudes over twelve decades (a tolerance from the tensor's maximum would hide a wrong weight on a small pixel); plane (0, 0) is
    a ramp in x plus another in y around zero, on which every output is exactly representable."""
    B, C, H, W = shape
    rng = np.random.default_rng(_seed_of(shape, 4))
    x = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 6, shape)).astype(np.float32)
    x[0, 0] = ramp(H, W)
    return {'x': frozen(x), 'slope': frozen(slopes(C, B + C + H))}


def ramp(H, W):
    """3 x - 5 y + 40 less the middle: small integers, so that the weights 0, 0.25, 0.75, 1 and the power-of-two slopes give exact values."""
    ys, xs = np.arange(H, dtype=np.float32)[:, None], np.arange(W, dtype=np.float32)[None, :]
    return (3 * xs - 5 * ys - np.float32(3 * (W // 2) - 5 * (H // 2))).astype(np.float32)


def _source(n_out, n_in, dtype):
    """source = max(0.5 (dst + 0.5) - 0.5, 0) -> (index, its neighbour clamped at the edge, weight of the index, weight of the neighbour)"""
    pos = np.maximum(dtype(0.5) * (np.arange(n_out).astype(dtype) + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = pos.astype(np.int64)
    l1 = (pos - i0.astype(dtype)).astype(dtype)
    return i0, np.minimum(i0 + 1, n_in - 1), (dtype(1) - l1).astype(dtype), l1


@_quiet
def upsample_reference(x, slope=None, dtype=np.float64, swap_columns=False):
    """The kernel's own definition, h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11) and the PReLU, in `dtype` -> (out [B,C,2H,2W], M: the largest
    magnitude among each output's four taps).  In float64 every step is exact to 2^-53: the value.  In float32 it is the kernel's arithmetic
    restated.  swap_columns: the mutant that exchanges the two column weights."""
    B, C, H, W = x.shape
    v = np.asarray(x, dtype=np.float32).astype(dtype)
    y0, y1, h0, h1 = _source(2 * H, H, dtype)
    x0, x1, w0, w1 = _source(2 * W, W, dtype)
    if swap_columns:
        w0, w1 = w1, w0
    h0, h1 = h0[:, None], h1[:, None]
    v00, v01, v10, v11 = v[:, :, y0][:, :, :, x0], v[:, :, y0][:, :, :, x1], v[:, :, y1][:, :, :, x0], v[:, :, y1][:, :, :, x1]
    out = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)
    if slope is not None:
        out = prelu(out, _per_channel(slope, dtype))
    M = np.maximum(np.maximum(np.abs(v00), np.abs(v01)), np.maximum(np.abs(v10), np.abs(v11))).astype(np.float64)
    return out.astype(dtype), M


def upsample_bound(M, slope=None):
    """Per output element, M the largest magnitude among its four taps.  The weights are exact, so to first order the four products, the two
    inner sums, the two outer products and the last sum leave 4 u M (each of the two chains product, sum, product rounds three values of at
    most M, weighted by h0 + h1 = 1, and the last sum one more): 5 u M is allowed, and (1 + |slope|) 5 u M under a PReLU, which covers a
    rounding that crosses zero (one side of it is scaled by the slope, the other is not)."""
    bound = 5 * U * M
    return bound if slope is None else bound * (1 + np.abs(np.asarray(slope, dtype=np.float64)).reshape(1, -1, 1, 1))


# ---------------------------------------------------------------------------------------
# the grid limits
# ---------------------------------------------------------------------------------------

MAX_PLANES, MAX_OUT_ROWS = 65535, 65535                         # B C and 2 H: a grid's y and z extents
BIAS_ACT_AT_LIMIT = [(1, MAX_PLANES, 1, 4), (1, MAX_PLANES, 1, 3)]      # the vector and the scalar path
UPSAMPLE_AT_LIMIT = [(1, MAX_PLANES, 1, 1), (1, 1, MAX_OUT_ROWS // 2, 1)]
BIAS_ACT_ABOVE = [(1, MAX_PLANES + 1, 1, 4), (256, 256, 1, 3)]
UPSAMPLE_ABOVE = [(1, MAX_PLANES + 1, 1, 1), (1, 1, MAX_OUT_ROWS // 2 + 1, 1)]
CALLER_BATCH = (256, 256, 2, 2)                                 # B C = 65536 on the GridNet's 256-channel row


@functools.lru_cache(maxsize=None)
def limit_inputs(shape):
    B, C, H, W = shape
    rng = np.random.default_rng(_seed_of(shape, 5))
    period = 7                                                  # slopes and biases that differ between neighbouring channels, every plane its own values
    return {'x': frozen(rng.standard_normal(shape).astype(np.float32)), 'bias': frozen(rng.standard_normal(C).astype(np.float32)),
            'slope': frozen((np.arange(C) % period).astype(np.float32) * np.float32(0.125) - np.float32(0.25)),
            'res1': frozen(rng.standard_normal(shape).astype(np.float32))}
