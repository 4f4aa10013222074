"""NumPy restatement of the device's vector algebra and scalar reductions (include/fwi.h: fwi_vec_dot, fwi_dot,
fwi_misfit_l2, fwi_vec_axpby / mul / recip / clip / absmax), kept apart from the package.

The two sums are restated in the ORDER the kernels add in, so that their result can be compared bit for bit:

    blocks = min(1024, ceil(n / 256)) blocks of 256 threads over the compact array of n elements;
    1. thread g (= 256 block + t) adds its products over the ascending indices g, g + 256 blocks, ... (from +0);
    2. a wave adds its 64 lanes by the tree  lane l += lane l + off,  off = 32, 16, .., 1;
    3. a block adds its four waves as (w0 + w1) + (w2 + w3): the block partial;
    4. one block of 256 threads adds the partials: thread t adds partial t, t + 256, .. in ascending order (from +0),
       and the 256 results go through the tree  t += t + s,  s = 128, 64, .., 1.

The products are formed in fp64.  Of fp32 inputs they are exact (48 bits at most), so a contraction of the multiply
and the add into an FMA changes nothing and the restatement is exact arithmetic in a known order; with fp64 inputs it
is to be used only where the products are exact, too (fp32-representable values held as fp64).  An index past n adds
+0, which changes no accumulator (none can be -0: they start at +0).

The element-wise operations are plain fp64 NumPy."""
import math

import numpy as np

BLOCK, WAVE, MAX_BLOCKS = 256, 64, 1024


def cx_of(nx):
    """Row stride of the compact layout: nx rounded up to a multiple of 4."""
    return (int(nx) + 3) // 4 * 4


def compact(a, shape):
    """The array as the device holds it: rows of the last axis padded with zeros to cx, flattened."""
    a = np.asarray(a).reshape(shape)
    out = np.zeros(tuple(shape[:-1]) + (cx_of(shape[-1]),), a.dtype)
    out[..., :shape[-1]] = a
    return out.ravel()


def sum_blocks(n):
    return max(1, min(MAX_BLOCKS, (int(n) + BLOCK - 1) // BLOCK))


def block_partials(terms):
    """Steps 1-3: the block partials of the fp64 terms (one per element of the flat array the kernel runs over)."""
    terms = np.asarray(terms, np.float64).ravel()
    blocks = sum_blocks(terms.size)
    threads = blocks * BLOCK
    trips = max(1, (terms.size + threads - 1) // threads)
    t = np.zeros(trips * threads)
    t[:terms.size] = terms
    t = t.reshape(trips, threads)
    acc = np.zeros(threads)
    for k in range(trips):
        acc = acc + t[k]
    v = acc.reshape(blocks, BLOCK // WAVE, WAVE).copy()
    off = WAVE // 2
    while off:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    w = v[..., 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def final_sum(partials):
    """Step 4: the total of the block partials."""
    partials = np.asarray(partials, np.float64).ravel()
    rows = max(1, (partials.size + BLOCK - 1) // BLOCK)
    p = np.zeros(rows * BLOCK)
    p[:partials.size] = partials
    p = p.reshape(rows, BLOCK)
    acc = np.zeros(BLOCK)
    for k in range(rows):
        acc = acc + p[k]
    s = BLOCK // 2
    while s:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return float(acc[0])


def products(a, b, shape=None):
    """The fp64 products the kernel adds: over the compact layout of ``shape``, or over the flat arrays as they are
    (``shape=None``: fwi_dot)."""
    a, b = np.asarray(a), np.asarray(b)
    if shape is not None:
        a, b = compact(a, shape), compact(b, shape)
    return a.ravel().astype(np.float64) * b.ravel().astype(np.float64)


def dot_bits(a, b, shape=None):
    """sum a b in the kernel's order, as the fp64 value the device returns."""
    return final_sum(block_partials(products(a, b, shape)))


def sumsq_bits(r):
    """sum r^2 of the flat residual in the kernel's order (fwi_misfit_l2 returns half of it)."""
    r = np.asarray(r).ravel().astype(np.float64)
    return final_sum(block_partials(r * r))


def dot_fsum(a, b):
    """(the correctly rounded sum of the fp64 products, sum |a b|) of the logical elements"""
    p = np.asarray(a).ravel().astype(np.float64) * np.asarray(b).ravel().astype(np.float64)
    return math.fsum(p.tolist()), math.fsum(np.abs(p).tolist())


def sum_bound(n, sum_abs, product_rounding=False):
    """Any order of n terms: 1.01 n 2^-53 sum |terms|; one more rounding each where the fp64 products are not exact."""
    return 1.01 * (n + (1 if product_rounding else 0)) * 2.0 ** -53 * sum_abs


def wide(rng, shape, dtype=np.float32):
    """standard_normal * 10 ** uniform(-3, 3): six decades of magnitudes make the order of a sum visible in its last
    bits.  Read-only."""
    a = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)).astype(np.float32).astype(dtype)
    a.setflags(write=False)
    return a


# ---- element-wise references: fp64, from the definition --------------------------------------------------------
def axpby(a, x, b, y):
    """a x + b y in fp64 (IEEE: 0 * NaN and 0 * inf are NaN)."""
    with np.errstate(all="ignore"):
        return a * np.asarray(x, np.float64) + b * np.asarray(y, np.float64)


def axpby_bound(a, x, b, y, dtype):
    """fp64 arithmetic (two products, one sum) and one rounding to T: u_T |ref| + 3 2^-53 (|a x| + |b y|), and T's
    smallest normal number where the result is below the normal range."""
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    with np.errstate(all="ignore"):
        ax, by = np.abs(a * np.asarray(x, np.float64)), np.abs(b * np.asarray(y, np.float64))
        return u * np.abs(axpby(a, x, b, y)) + 3.0 * 2.0 ** -53 * (ax + by) + float(np.finfo(dtype).tiny)


def mul(x, y):
    """The product in the arrays' own type (the fp64 product of two T rounded once to T is the product in T)."""
    with np.errstate(all="ignore"):
        return np.asarray(x) * np.asarray(y)


def recip(y, a, b):
    with np.errstate(all="ignore"):
        return a / (np.asarray(y, np.float64) + b)


def recip_bound(y, a, b, dtype):
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    return (u + 3.0 * 2.0 ** -53) * np.abs(recip(y, a, b))


def clip(x, lo, hi):
    return np.clip(np.asarray(x), lo, hi)


def absmax(x):
    return float(np.abs(np.asarray(x)).max())


def same_bits(a, b):
    """Equal bit patterns, element by element (NaN payloads, the sign of zero and denormals included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the cases the CPU and the GPU suite share -------------------------------------------------------------------
# grid shapes, each the smallest instance of a property (cx = row stride, cells = compact elements):
SHAPES = [
    (9, 5, 1),        # cx 4, 180 cells: three quarters of every row is pad
    (5, 7),           # cx 8, 40 cells: less than one wave
    (8, 32),          # cx 32, 256 cells: exactly one block, no pad
    (8, 33),          # cx 36, 288 cells: a second, mostly idle block; two partials
    (20, 17, 23),     # cx 24: 3-D with pad
    (520, 509),       # cx 512, 266,240 cells: past the 1024 x 256 cap of the sums: two trips, all 1024 partials
    (1030, 1021),     # cx 1024, 1,054,720 cells: past the 2048 x 256 cap of the element-wise launches and the
                      # 4096 x 256 cap of repack
]
LARGE_SHAPES = SHAPES[-2:]  # the ones whose inputs must make the order of the block partials visible
DOT_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 262144, 262145, 1000003]  # fwi_dot, host arrays unrelated to the grid
LARGE_DOT_SIZES = DOT_SIZES[-3:]

# seeds at which at least 90 of 100 random orders of the block partials change the bits of the total
# (tests/test_vecops_host.py checks it): the condition is on the inputs, so a case that misses it gets another seed
SEEDS = {(520, 509): 4, (1030, 1021): 2, 262144: 4, 262145: 8, 1000003: 6}
_cache = {}


def vec_pair(shape, dtype=np.float32):
    """The two wide-range vectors of a grid shape: fp32 values, held as ``dtype`` (so fp64 products are exact too)."""
    key = ("vec", tuple(shape))
    if key not in _cache:
        rng = np.random.default_rng([SEEDS.get(tuple(shape), 7)] + list(shape))
        _cache[key] = (wide(rng, shape), wide(rng, shape))
    a, b = _cache[key]
    if np.dtype(dtype) == np.float32:
        return a, b
    out = a.astype(dtype), b.astype(dtype)
    for o in out:
        o.setflags(write=False)
    return out


def flat_pair(n, dtype=np.float32):
    key = ("flat", int(n))
    if key not in _cache:
        rng = np.random.default_rng([SEEDS.get(int(n), 11), int(n)])
        _cache[key] = (wide(rng, int(n)), wide(rng, int(n)))
    a, b = _cache[key]
    if np.dtype(dtype) == np.float32:
        return a, b
    out = a.astype(dtype), b.astype(dtype)
    for o in out:
        o.setflags(write=False)
    return out


def orders_that_change_the_bits(partials, trials=100, seed=5):
    """Of ``trials`` random orders of the block partials, how many give a total with other bits than the kernel's
    order does."""
    rng = np.random.default_rng(seed)
    partials = np.asarray(partials, np.float64)
    ref = final_sum(partials)
    return sum(final_sum(rng.permutation(partials)) != ref for _ in range(trials))


def cancelling_pair(shape):
    """(x, y) on a grid whose rows are two blocks long (cx = 512): odd integers in the first half of every row, the
    same again in the second half, and y = +1 / -1 on the halves.  Every product is an exact integer, the partial of
    block 2k + 1 is the negative of that of block 2k, none is zero (253 odd numbers), and the total is exactly 0."""
    nx = shape[-1]
    assert len(shape) == 2 and cx_of(nx) == 512 and nx > 256
    rng = np.random.default_rng(3)
    v = (2 * rng.integers(-2 ** 19, 2 ** 19, (shape[0], 256)) + 1).astype(np.float32)
    v[:, nx - 256:] = 0.0  # the cells whose partner would be a pad column
    x = np.concatenate([v, v[:, :nx - 256]], axis=1)
    y = np.concatenate([np.ones((shape[0], 256), np.float32), -np.ones((shape[0], nx - 256), np.float32)], axis=1)
    for a in (x, y):
        a.setflags(write=False)
    return x, y


def special_values(shape, dtype):
    """Ordinary values on both sides of the clip ranges the tests use, with a -0.0, a +0.0 and denormals of both signs
    among them.  A fresh, writeable array."""
    rng = np.random.default_rng(13)
    x = rng.uniform(-3.0, 3.0, shape).astype(dtype)
    flat = x.reshape(-1)
    tiny = np.finfo(dtype).smallest_subnormal
    for k, v in enumerate((-0.0, 0.0, tiny, -tiny, 3 * tiny, np.finfo(dtype).tiny / 2)):
        flat[(7 * k + 3) % flat.size] = v
    return x


def plant_cells(shape):
    """Where a maximum or a NaN is planted, in turn: the first cell, the last logical cell, the last cell of a row before
    its pad columns, and an interior cell -- of the largest shape one that the element-wise launches (2048 blocks of
    256) and the sums reach only in a later trip of their grid-stride loop."""
    first = (0,) * len(shape)
    last = tuple(s - 1 for s in shape)
    row_end = (0,) * (len(shape) - 1) + (shape[-1] - 1,)
    inner = tuple(s * 3 // 5 for s in shape)
    if int(np.prod(shape[:-1])) * cx_of(shape[-1]) > 2048 * 256:
        assert np.ravel_multi_index(inner[:-1], shape[:-1]) * cx_of(shape[-1]) + inner[-1] >= 2048 * 256
    return [first, last, row_end, inner]
