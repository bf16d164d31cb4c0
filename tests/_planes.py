"""The fp16-plane format stated in numpy float32 / float16 arithmetic, from include/pylc_hip.h ("fp16 planes", precision mode 2) and
DESIGN.md sections 4 / 5.1 (not from the kernels), with the derived error bounds tests/test_planes_abi_gpu.py uses and the inputs both
that file and tests/test_cpu_planes_ref.py run on.  Not a test module.

The format.  A range scalar holds the IEEE bits of a float `bound` >= max|x|.  s = scale_for(bits) is the power of two that maps the bound
into [2^14, 2^15): exponent field of s = 127 + 14 - (e - 127), e the exponent field of the bound, clamped to 1..242 (s <= 2^115: the
split multiplies it by 2^11, which must stay finite).  v = s x is exact (a power-of-two scale; |v| < 2^15).  The pieces are
    h0 = rn16(v)                    h1 = rn16(2^11 (v - h0))                    x ~ ((float)h0 + (float)h1 / 2048) / s
with rn16 = round to nearest even to fp16, subnormals kept (numpy's astype(float16)).  One-plane tensors hold h0 only.
The sign of a ZERO piece is not part of the format (include/pylc_hip.h): for x = -0 the model has h0 = -0, h1 = +0, the kernels may store
h1 = -0 (the compiler forms the rn16(s x) that the residual is taken against as a fused multiply-add with a +0 addend, so -0 - +0 = -0).
Every comparison of pieces goes through canon(), which clears the sign of zeros and nothing else.

The bounds (in units of v; divide by s for x).
  * Two planes.  r = v - h0 is exact in fp32 (|r| <= half an fp16 ulp of v, and a multiple of the fp32 ulp of v).  v has 24 significant
    bits and h0 takes the leading 11, so r has at most 13, the lowest at 2^-23 of v's leading bit.  If 2^11 r is an fp16 NORMAL, h1 keeps
    11 of those bits: what it can drop lies at or below that lowest position, and a half-way case rounds by exactly one such unit -- error
    <= 2^-23 |v|, attained at ties.  If 2^11 r is an fp16 SUBNORMAL (|2^11 r| < 2^-14) the rounding unit is fixed: error <= 2^-25 in
    h1, 2^-36 in v, attained at ties.  Hence   |h0 + 2^-11 h1 - v| <= max(2^-23 |v|, 2^-36);   the floor is the larger one exactly for
    |v| < 2^-13, i.e. for |x| below 2^-27 .. 2^-28 of the bound, and it is 2^-50 .. 2^-51 of the bound.
  * One plane.  Half an ulp of h0: 2^-11 |v| while v is an fp16 normal, 2^-25 below:   |h0 - v| <= max(2^-11 |v|, 2^-25).
  * The rebuilt sum h0 + 2^-11 h1 is exact in fp32: both terms are multiples of the fp32 ulp of v or of 2^-35, and the sum approximates v
    to better than that ulp (join_is_exact() checks it in float64).  The division by s is exact unless the result is an fp32 subnormal:
    a round trip through fp32 then adds at most half the subnormal spacing, 2^-150 (round_trip_bound).
  * Per-channel sums and means read from planes.  A sum of n fp32 terms in ANY order makes at most n - 1 roundings, each of a partial sum
    no larger than sum|x|; the fp64 combine of slab partials is rounded to fp32 once more: <= n 2^-24 sum|x| to first order.  The mean
    divides that by n (the two further roundings of the mean itself, each 2^-24 |mean|, are not added: the figure is already loose by
    about sqrt(n)).  One dropped or doubled row changes a channel's sum by sum|x| / n on average, n^2 2^-24 times less than the bound
    allows: 0.03 and below for the shapes of the GPU tests except the 4100-row column sum, where the two are equal (n^2 2^-24 = 1.002).
"""
import numpy as np

F32, F16 = np.float32, np.float16
FILL16 = 0x7e00                       # the fp16 NaN pattern half buffers are filled with


def bits_of(v):
    return int(np.array([v], dtype=F32).view(np.uint32)[0])


def float_of(bits):
    return np.array([bits], dtype=np.uint32).view(F32)[0]


def scale_for(bits):
    """The header's rule: the power of two (as np.float32) that maps the bound behind `bits` into [2^14, 2^15), exponent field 1..242."""
    e = (int(bits) >> 23) & 0xFF
    se = min(max(127 + 14 - (e - 127), 1), 242)
    return float_of(se << 23)


def split(x, s):
    """(h0, h1) of fp32 values x under the scale s, every operation in fp32 / fp16 as the header states it."""
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.asarray(x, dtype=F32) * F32(s)
        h0 = v.astype(F16)
        h1 = ((v - h0.astype(F32)) * F32(2048.0)).astype(F16)
    return h0, h1


def join(h0, h1, s):
    """((float)h0 + (float)h1 / 2048) / s in fp32; h1 = None for a one-plane tensor."""
    acc = h0.astype(F32)
    if h1 is not None:
        acc = acc + h1.astype(F32) / F32(2048.0)
    return acc / F32(s)


def join_is_exact(h0, h1):
    """The fp32 sum h0 + h1 / 2048 equals the float64 one."""
    a = h0.astype(F32) + h1.astype(F32) / F32(2048.0)
    return bool(np.array_equal(a.astype(np.float64), h0.astype(np.float64) + h1.astype(np.float64) / 2048.0))


def canon(u16):
    """uint16 fp16 patterns with -0 (0x8000) replaced by +0: a zero piece may carry either sign."""
    u16 = np.asarray(u16, dtype=np.uint16)
    return np.where(u16 == 0x8000, np.uint16(0), u16)


def phys(e, interleaved):
    """Address (halves) of plane 0 of flat element e; chunk-interleaved: (e >> 5) * 64 + (e & 31), plane 1 at + 32."""
    e = np.asarray(e, dtype=np.int64)
    return (e >> 5) * 64 + (e & 31) if interleaved else e


def place(h0, h1, interleaved, out=None, base=0, stride=None, index=None):
    """Write the pieces of a flat tensor into a uint16 buffer the way the format lays them out: element i at base + phys(index[i]) (index:
    default arange), plane 1 at + 32 (interleaved) or + stride (separate; default: the element count).  h1 = None: plane 0 only."""
    n = h0.size
    index = np.arange(n, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64).ravel()
    if stride is None:
        stride = n
    if out is None:
        out = np.zeros(2 * n if h1 is not None else n, dtype=np.uint16)
    at = base + phys(index, interleaved)
    out[at] = h0.ravel().view(np.uint16)
    if h1 is not None:
        out[at + (32 if interleaved else stride)] = h1.ravel().view(np.uint16)
    return out


def filter_planes(w, s, interleave):
    """Prepared planes of a filter w[K][RS][C] (pylc_weight_prepare): (forward [2][K][RS][C], transposed [2][C][RS][Kp]) as uint16 arrays,
    Kp = roundup4(K) with zero pad columns; each layout chunk-interleaved iff `interleave` and its channel count (C resp. Kp) % 32 == 0."""
    w = np.asarray(w, dtype=F32)
    K, RS, C = w.shape
    Kp = (K + 3) & ~3
    h0, h1 = split(w, s)
    fwd = place(h0, h1, bool(interleave) and C % 32 == 0)
    t0, t1 = np.zeros((C, RS, Kp), dtype=F16), np.zeros((C, RS, Kp), dtype=F16)
    t0[:, :, :K] = h0.transpose(2, 1, 0)
    t1[:, :, :K] = h1.transpose(2, 1, 0)
    return fwd, place(t0, t1, bool(interleave) and Kp % 32 == 0)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------
def bound2(x, s):
    """Two planes, per element, in units of x (float64)."""
    return np.maximum(2.0 ** -23 * np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -36 / float(s))


def bound1(x, s):
    """One plane, per element, in units of x (float64)."""
    return np.maximum(2.0 ** -11 * np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -25 / float(s))


def round_trip_bound(x, s, nplanes):
    """bound2 / bound1 plus the half spacing 2^-150 of fp32 subnormals where the rebuilt fp32 value can be one (|x| < 2^-125)."""
    b = bound2(x, s) if nplanes == 2 else bound1(x, s)
    return b + np.where(np.abs(np.asarray(x, dtype=np.float64)) < 2.0 ** -125, 2.0 ** -150, 0.0)


def floor_share(x, s, nplanes=2):
    """Share of the elements whose bound is the absolute floor."""
    v = np.abs(np.asarray(x, dtype=np.float64)) * float(s)
    return float(np.mean(v < (2.0 ** -13 if nplanes == 2 else 2.0 ** -14)))


def sum_bound(x, axis=0):
    """Any-order fp32 sum over `axis` of n terms: n 2^-24 sum|x| (float64)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return x.shape[axis] * 2.0 ** -24 * x.sum(axis)


def mean_bound(x, axis=0):
    return sum_bound(x, axis) / np.asarray(x).shape[axis]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def wide(seed, M, C):
    """[M][C] fp32, N(0, 1) x 2^U(-45, 0): about half the elements below the relative window of a bound at the maximum."""
    r = np.random.RandomState(seed)
    return (r.standard_normal((M, C)) * 2.0 ** r.uniform(-45.0, 0.0, (M, C))).astype(F32)


# scaled values v = s x to plant (all |v| <= 2, below s max|x| for every range scalar up to 2^12 x the maximum)
_T = 2.0 ** -24                     # the fp16 subnormal spacing
SPECIAL_V = (
    0.0, -0.0,
    1.0, -2.0 ** -5, 2.0 ** -20, 2.0 ** -30,                             # exact powers of two (normal h0; subnormal h0; h0 = 0)
    1.0 + 2.0 ** -11, -(1.0 + 2.0 ** -11), 1.0 + 3 * 2.0 ** -11,         # h0 half-way: to the even neighbour below (1) resp. above (1 + 2^-9)
    1.0 + 2.0 ** -12 + 2.0 ** -23, 1.0 + 2.0 ** -12 + 3 * 2.0 ** -23,    # 2^11 r half-way (normal h1): down to 0.5, up to 0.5 (1 + 2^-9); error = 2^-23 |v|
    5.5 * _T, 6.5 * _T, -2.5 * _T,                                       # subnormal h0 at a tie: 6, 6, -2 spacings
    3 * _T + 2.0 ** -26,                                                 # subnormal h0 and subnormal h1, both exact
    2.0 ** -14 + 2.0 ** -36, 2.0 ** -14 + 3 * 2.0 ** -36,                # smallest normal h0; 2^11 r = 0.5, 1.5 subnormal spacings: ties to 0 and to 2 (error = the floor)
    2.0 ** -14 + 3 * 2.0 ** -37,                                         # ... 0.75 spacings: h1 = one spacing
    2.0 ** -20 + 3 * 2.0 ** -37,                                         # both pieces subnormal, h1 rounded
    2.0 ** -13, -2.0 ** -13, 2.0 ** -13 * (1.0 + 2.0 ** -23),            # the edge of the relative window, and its fp32 neighbour
)


def plant(x, mult=1.0, bits=None):
    """A copy of x[M][C] with the edge values planted at fixed pseudo-random places, for the range scalar `mult` (a power of two) x max|x|
    (or the given `bits`, a bound of a larger tensor x is a part of): +- the maximum, and every SPECIAL_V whose x = v / s is an fp32 number
    (for a tiny bound some are not and are left out).  In a tensor too small for all of them the first ones win.  Returns (x, bits of the
    range scalar)."""
    x = np.array(x, dtype=F32)
    flat = x.reshape(-1)
    amax = F32(np.abs(flat).max())
    if bits is None:
        bits = bits_of(F32(amax * F32(mult)))
    s = scale_for(bits)
    vals = [amax, -amax]
    for v in SPECIAL_V:
        xv = F32(F32(v) / s)
        if float(F32(v)) == v and float(xv) * float(s) == v and np.signbit(xv) == np.signbit(F32(v)):
            vals.append(xv)
    where = np.random.RandomState(flat.size).permutation(flat.size)[:len(vals)]
    flat[where] = np.array(vals[:where.size], dtype=F32)
    return x, bits
