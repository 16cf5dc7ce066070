"""Grid rows of the packed copy (common.h: kPackedGrid) restated in numpy: the membership rule of
k_pack_rows, the fixed-point lo / hi planes it writes and the decode of octet_reduce_packed_grid (insert the magnitude into
the bits of 2^(e_max + 1), subtract 2^(e_max + 1), insert the sign), lane order included.  A grid row round-trips bit for
bit through the grid codec, every other row through the 28-bit codec of test_packed_rows_cpu (or is raw).  No GPU."""
import numpy as np

from test_packed_rows_cpu import RAW, layout, pack_row, unpack_row

GRID = 0x200
E_MIN, E_MAX = 25, 253


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def is_grid(x):
    """The rule: 25 <= e_max <= 253, no inf / NaN, every element +-0 or normal with the low e_max - e + 1 bits of its
    24-bit significand clear (which also keeps e >= e_max - 22).  Written element by element, as the issue states it."""
    b = u32(x).astype(np.int64)
    e = (b >> 23) & 255
    man = b & 0x7FFFFF
    emax = int(e.max())
    if not E_MIN <= emax <= E_MAX or (e == 255).any():
        return False
    if ((e == 0) & (man != 0)).any():  # a non-zero denormal
        return False
    nz = e != 0
    sh = emax - e[nz] + 1
    if (sh > 23).any():  # e < e_max - 22
        return False
    sig = man[nz] | 0x800000
    return bool(((sig & ((1 << sh) - 1)) == 0).all())


def is_grid_lowbit(x):
    """The same rule the way k_pack_rows computes it in one pass: min over normal elements of e + ctz(significand)."""
    b = u32(x).astype(np.int64)
    e = (b >> 23) & 255
    emax = int(e.max())
    if not E_MIN <= emax <= E_MAX or (e == 255).any() or ((e == 0) & ((b & 0x7FFFFF) != 0)).any():
        return False
    sig = (b & 0x7FFFFF) | 0x800000
    ctz = np.log2((sig & -sig).astype(np.float64)).astype(np.int64)
    low = np.where(e != 0, e + ctz, 1 << 16).min()
    return bool(low >= emax + 1)


def pack_grid(x):
    """(row_exp, lo + hi plane bytes) of a grid row: no code plane."""
    assert is_grid(x)
    b = u32(x).astype(np.int64)
    blocks = b.size // 32
    b8 = (blocks + 7) // 8 * 8
    pb = np.zeros(b8 * 32, dtype=np.int64)
    pb[:b.size] = b
    e = (pb >> 23) & 255
    emax = int(e.max())
    mag = np.where(e == 0, 0, ((pb & 0x7FFFFF) | 0x800000) >> np.where(e == 0, 0, emax - e + 1))
    assert (mag < (1 << 23)).all()
    lo16 = mag & 0xFFFF
    hi8 = ((pb >> 24) & 0x80) | (mag >> 16)
    lo = lo16.reshape(b8 // 2, 2, 8, 4).transpose(0, 2, 1, 3).reshape(-1).astype("<u2").tobytes()
    hi = hi8.reshape(b8 // 4, 4, 8, 4).transpose(0, 2, 1, 3).reshape(-1).astype(np.uint8).tobytes()
    n_lo, n_hi, _ = layout(blocks)
    assert not any(lo[128 * n_lo:]) and not any(hi[128 * n_hi:])
    return emax | GRID, lo[:128 * n_lo] + hi[:128 * n_hi]


def grid_decode(a, emax):
    """grid_value on the v_perm result a = lo16 | hi byte << 16 | hi byte << 24, in f32 arithmetic."""
    two = np.uint32((emax + 1) << 23)
    r = (a & np.uint32(0x007FFFFF)) | two                       # v_bfi: magnitude into the bits of 2^(e_max + 1)
    f = r.view(np.float32) - np.array(two).view(np.float32)     # exact
    return (a & np.uint32(0x80000000)) | (np.ascontiguousarray(f, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF))


def unpack_grid(row_exp, planes, dims):
    assert row_exp & GRID
    blocks = dims // 32
    b8 = (blocks + 7) // 8 * 8
    n_lo, n_hi, _ = layout(blocks)
    assert len(planes) == 128 * (n_lo + n_hi)  # the bytes up to code_off, nothing of the code plane
    p = np.frombuffer(planes, dtype=np.uint8)
    pad = lambda a, n: np.concatenate([a, np.zeros(n - a.size, dtype=np.uint8)])
    lo = pad(p[:128 * n_lo], b8 * 64).view("<u2").astype(np.uint32).reshape(b8 // 2, 8, 2, 4).transpose(0, 2, 1, 3).reshape(-1)
    hi = pad(p[128 * n_lo:], b8 * 32).astype(np.uint32).reshape(b8 // 4, 8, 4, 4).transpose(0, 2, 1, 3).reshape(-1)
    a = (lo | (hi << 16) | (hi << 24)).astype(np.uint32)
    return grid_decode(a, row_exp & 0xFF)[:dims].view(np.float32)


def roundtrip(x):
    """'grid', 'packed' or 'raw': how the row is stored; whichever codec stores it gives back every bit."""
    x = np.asarray(x, dtype=np.float32)
    assert is_grid(x) == is_grid_lowbit(x)
    if is_grid(x):
        rexp, planes = pack_grid(x)
        y = unpack_grid(rexp, planes, x.size)
        assert np.array_equal(u32(y), u32(x)), np.nonzero(u32(y) != u32(x))[0][:5]
        return "grid"
    rexp, planes = pack_row(x)
    if rexp == RAW:
        return "raw"
    assert np.array_equal(u32(unpack_row(rexp, planes, x.size)), u32(x))
    return "packed"


def policy_normal(rng, shape):
    """the policy generator's N(0,1): twelve 20-bit uniforms minus 6, a multiple of 2^-20"""
    return ((rng.integers(0, 1 << 20, size=shape + (12,)).sum(axis=-1) - 6 * (1 << 20)) / float(1 << 20)).astype(np.float32)


def uniform_pm1(rng, shape):
    """24-bit uniforms mapped to [-1, 1): multiples of 2^-23"""
    return ((rng.integers(0, 1 << 24, size=shape) - (1 << 23)) / float(1 << 23)).astype(np.float32)


def test_members_roundtrip():
    rng = np.random.default_rng(3)
    for dims in (32, 96, 640, 768, 1536):
        for _ in range(10):
            x = uniform_pm1(rng, (dims,))
            x[x == -1.0] = 0.5
            x[0] = np.float32(0.75)  # e_max = 126 for sure
            assert roundtrip(x) == "grid"
            assert roundtrip(policy_normal(rng, (dims,))) == "grid"
            # f32 casts of bf16 values: 8 significant bits, so a spread of up to 15 binades fits
            y = rng.standard_normal(dims).astype(np.float32)
            y = (u32(y) & np.uint32(0xFFFF0000)).view(np.float32).copy()
            y[np.abs(y) < np.abs(y).max() * 2.0 ** -14] = np.abs(y).max()
            assert roundtrip(y) == "grid"
            assert roundtrip(y * np.float32(2.0 ** 90)) == "grid" and roundtrip(y * np.float32(2.0 ** -90)) == "grid"


def test_members_with_zeros_and_deep_elements():
    base = uniform_pm1(np.random.default_rng(4), (96,))
    base[base == -1.0] = 0.5
    base[0] = np.float32(0.75)
    x = base.copy()
    x[3], x[4] = 0.0, -0.0
    assert roundtrip(x) == "grid"
    rexp, planes = pack_grid(x)
    y = unpack_grid(rexp, planes, 96)
    assert u32(y)[3] == 0 and u32(y)[4] == 0x80000000  # the sign of -0 is kept
    x = base.copy()
    x[7] = np.float32(-(2.0 ** -21))   # 20 binades below e_max = 126 (a multiple of the unit 2^-23): raw in the 28-bit rule
    assert pack_row(x)[0] == RAW and roundtrip(x) == "grid"
    x[8] = np.float32(2.0 ** -23)      # 22 binades down, the unit itself: the deepest member
    assert roundtrip(x) == "grid"


def test_non_members():
    rng = np.random.default_rng(5)
    half = (rng.integers(1 << 23, 1 << 24, size=64) / float(1 << 24)).astype(np.float32)  # [0.5, 1), multiples of 2^-24
    half[::2] = (u32(half[::2]) | np.uint32(1)).view(np.float32)                           # ... odd ones among them
    x = half.copy()
    x[5] = np.float32(-1.0)  # e_max becomes 127: the odd multiples of 2^-24 lose a bit; and -1.0 beside multiples of 2^-23
    assert not is_grid(x) and roundtrip(x) == "packed"
    y = uniform_pm1(rng, (64,))
    y[y == -1.0] = 0.5
    y[0] = np.float32(0.75)
    y[1] = np.float32(0.5 + 2.0 ** -23)  # an odd multiple of the unit 2^-23 in [0.5, 1)
    assert roundtrip(y) == "grid"
    y[5] = np.float32(-1.0)              # e_max 127, unit 2^-22: the magnitude of y[1] would need a 24th bit
    assert not is_grid(y) and roundtrip(y) == "packed"
    u01 = (rng.integers(0, 1 << 24, size=(50, 768)) / float(1 << 24)).astype(np.float32)  # uniform[0,1): multiples of 2^-24
    assert not any(is_grid(r) for r in u01)
    full = rng.standard_normal((50, 768)).astype(np.float32)  # full-mantissa embeddings gain nothing
    assert not any(is_grid(r) for r in full)
    assert not any(is_grid(r / np.linalg.norm(r)) for r in full)
    ok = np.full(32, 1.5, dtype=np.float32)
    assert roundtrip(ok) == "grid"
    for bad in (np.float32(1e-40), np.float32(-1.4e-45)):  # a non-zero denormal
        x = ok.copy()
        x[9] = bad
        assert not is_grid(x) and roundtrip(x) == "packed"
    for bad in (np.inf, -np.inf, np.nan):
        x = ok.copy()
        x[9] = bad
        assert not is_grid(x) and roundtrip(x) == "raw"
    # e_max below 25 / above 253: the unit would be a denormal / 2^(e_max + 1) not finite
    assert roundtrip(np.full(32, 1.5 * 2.0 ** (24 - 127), dtype=np.float32)) == "packed"
    assert roundtrip(np.full(32, 1.5 * 2.0 ** (25 - 127), dtype=np.float32)) == "grid"
    assert roundtrip(np.full(32, 1.5 * 2.0 ** (253 - 127), dtype=np.float32)) == "grid"
    assert roundtrip(np.full(32, 1.5 * 2.0 ** (254 - 127), dtype=np.float32)) == "packed"
    assert roundtrip(np.zeros(32, dtype=np.float32)) == "packed"
    # an element 23 binades down has a set bit (its implicit one) below the unit
    x = ok.copy()
    x[2] = np.float32(2.0 ** -23)
    assert not is_grid(x) and roundtrip(x) == "raw"
    x[2] = np.float32(2.0 ** -22)  # 22 binades down: the unit
    assert roundtrip(x) == "grid"
    x[2] = np.float32(1.5 * 2.0 ** -22)  # ... with a bit below it
    assert not is_grid(x)


def test_subtract_trick_is_exact():
    """For several e_max: every magnitude with one bit set, with all bits set, and a random sample, both signs — the decode
    gives m x 2^(e_max - 149) exactly, and sign | 0 for m = 0."""
    rng = np.random.default_rng(6)
    m = np.concatenate([[0], 1 << np.arange(23), [(1 << 23) - 1], (1 << np.arange(1, 24)) - 1, rng.integers(0, 1 << 23, 4096)])
    for emax in (E_MIN, 26, 100, 126, 127, 128, 200, 252, E_MAX):
        for sign in (0, 1):
            a = (m | (sign << 31) | (sign << 23)).astype(np.uint32)  # bit 23 carries the hi byte's sign bit, as v_perm leaves it
            got = grid_decode(a, emax).view(np.float32)
            want = np.ldexp(m.astype(np.float64), emax - 149) * (-1.0 if sign else 1.0)
            assert np.array_equal(got.astype(np.float64), want), emax
            assert np.array_equal(np.signbit(got), np.full(m.size, bool(sign))), emax
            assert np.isfinite(got).all() and (np.abs(got[1:]) >= np.finfo(np.float32).tiny).all()


def test_bytes_read_per_grid_row():
    n_lo, n_hi, n_c = layout(768 // 32)
    assert 128 * (n_lo + n_hi) == 2304 and 128 * (n_lo + n_hi + n_c) == 2688  # 18 of the 21 pieces
