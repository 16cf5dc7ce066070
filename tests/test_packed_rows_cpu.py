"""The packed copy of the f32 rows (common.h: PackedView) restated in numpy: pack -> unpack gives back every
bit of a packed row, and a row is raw exactly where the rule says (an inf / NaN, or a normal element 15 or more binades
below the row's largest exponent).  Mirrors k_pack_rows / octet_reduce_packed, lane order included; no GPU."""
import numpy as np

RAW, ZEROS = 0xFF, 0x100


def layout(blocks):
    """pieces of the lo, hi and code planes (common.h: packed_layout): each plane only as long as its own pieces need"""
    return (blocks + 1) // 2, (blocks + 3) // 4, (blocks + 7) // 8


def pitch(dims):
    return 128 * sum(layout(dims // 32))


def pack_row(x):
    """(row_exp, planes bytes) of one row (dims % 32 == 0), or (RAW, None)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    e = (b >> 23) & 255
    normal = e != 0
    emax = int(e.max())
    if (e == 255).any() or (normal.any() and emax - int(e[normal].min()) >= 15):
        return RAW, None
    blocks = b.size // 32
    b8 = (blocks + 7) // 8 * 8  # (the arithmetic runs on whole groups of 8 blocks; each plane keeps only its live pieces)
    pb = np.zeros(b8 * 32, dtype=np.int64)
    pb[:b.size] = b
    pe = (pb >> 23) & 255
    lo16 = pb & 0xFFFF
    hi8 = ((pb >> 24) & 0x80) | ((pb >> 16) & 0x7F)
    code = np.where(pe == 0, 15, emax - pe)
    # element 32k + 4j + i of block k, lane j; pieces: lo 2 blocks, hi 4 blocks, code 8 blocks, each 8 lanes x 16 B
    lo = lo16.reshape(b8 // 2, 2, 8, 4).transpose(0, 2, 1, 3).reshape(-1).astype("<u2").tobytes()
    hi = hi8.reshape(b8 // 4, 4, 8, 4).transpose(0, 2, 1, 3).reshape(-1).astype(np.uint8).tobytes()
    c = code.reshape(b8 // 8, 8, 8, 4).transpose(0, 2, 1, 3).reshape(-1, 2)
    cb = (c[:, 0] | (c[:, 1] << 4)).astype(np.uint8).tobytes()
    n_lo, n_hi, n_c = layout(blocks)
    assert not any(lo[128 * n_lo:]) and not any(hi[128 * n_hi:])  # the cut pieces hold padding only
    lo, hi = lo[:128 * n_lo], hi[:128 * n_hi]
    return emax | (ZEROS if (pe[:b.size] == 0).any() else 0), lo + hi + cb


def unpack_row(row_exp, planes, dims):
    """The decode of octet_reduce_packed: v_perm [lo16, hi, hi], exponent (15 - c) + e_max - 15 (0 for code 15), v_bfi."""
    blocks = dims // 32
    b8 = (blocks + 7) // 8 * 8
    n_lo, n_hi, n_c = layout(blocks)
    p = np.frombuffer(planes, dtype=np.uint8)
    pad = lambda a, n: np.concatenate([a, np.zeros(n - a.size, dtype=np.uint8)])  # what the decode of dead pieces sees
    lo = pad(p[:128 * n_lo], b8 * 64).view("<u2").astype(np.uint32).reshape(b8 // 2, 8, 2, 4).transpose(0, 2, 1, 3).reshape(-1)
    hi = pad(p[128 * n_lo:128 * (n_lo + n_hi)], b8 * 32).astype(np.uint32)
    hi = hi.reshape(b8 // 4, 8, 4, 4).transpose(0, 2, 1, 3).reshape(-1)
    cb = p[128 * (n_lo + n_hi):].astype(np.uint32)
    assert cb.size == 128 * n_c == b8 * 16
    c = np.stack([cb & 15, cb >> 4], axis=1).reshape(b8 // 8, 8, 8, 4).transpose(0, 2, 1, 3).reshape(-1).astype(np.int64)
    emax = row_exp & 0xFF
    g = 15 - c
    e = ((g << 23) + ((emax - 15) << 23)) & 0xFFFFFFFF
    e = np.where(g == 0, 0, e) if row_exp & ZEROS else e
    a = lo | (hi << 16) | (hi << 24)
    out = (a & 0x807FFFFF) | (e & 0x7F800000)
    return out[:dims].astype(np.uint32).view(np.float32)


def roundtrip(x):
    x = np.asarray(x, dtype=np.float32)
    rexp, planes = pack_row(x)
    if rexp == RAW:
        return rexp
    assert len(planes) == pitch(x.size)
    y = unpack_row(rexp, planes, x.size)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32)), np.nonzero(y.view(np.uint32) != x.view(np.uint32))[0][:5]
    return rexp


def test_packed_bytes():
    rexp, planes = pack_row(np.random.default_rng(0).uniform(-1, 1, 768).astype(np.float32))
    assert rexp != RAW and len(planes) == 2688 == 21 * 128
    # bytes per row against the f32 row, and the automatic rule of ensure_packed: pitch + 2 <= 15/16 of 4 * dims
    assert [pitch(d) for d in (32, 64, 128, 256, 384, 640, 1536)] == [384, 384, 512, 896, 1408, 2304, 5376]
    pays = [d for d in range(32, 4097, 32) if 16 * (pitch(d) + 2) <= 15 * 4 * d]
    assert pays[:9] == [256, 384, 448, 480, 512, 640, 704, 736, 768]  # (not 128, 320 or 544: rounding eats the saving)
    assert all(d in pays for d in range(768, 4097, 256))


def test_roundtrip_random_rows():
    rng = np.random.default_rng(1)
    for dims in (32, 64, 96, 256, 288, 768, 1536):
        for _ in range(20):
            for x in (rng.uniform(-1, 1, dims), rng.standard_normal(dims) * 1e3, rng.standard_normal(dims) * 1e-30):
                x = x.astype(np.float32)
                x[np.abs(x) < np.abs(x).max() * 2.0 ** -13] = np.abs(x).max()  # keep the spread inside 14 binades: packed
                assert roundtrip(x) != RAW


def test_raw_rule_and_edges():
    base = np.full(64, 1.5, dtype=np.float32)  # exponent 127
    assert roundtrip(base) == 127  # a constant row
    for spread, raw in ((13, False), (14, False), (15, True), (16, True)):
        x = base.copy()
        x[7] = np.float32(2.0 ** -spread)  # exponent 127 - spread
        assert (roundtrip(x) == RAW) == raw, spread
    x = base.copy()
    x[3], x[4], x[40] = 0.0, -0.0, np.float32(-1e-40)  # ±0 and a denormal: code 15, not raw
    r = roundtrip(x)
    assert r != RAW and r & ZEROS
    assert roundtrip(np.zeros(32, dtype=np.float32)) == ZEROS  # e_max 0, all code 15
    for bad in (np.inf, -np.inf, np.nan):
        x = base.copy()
        x[9] = bad
        assert roundtrip(x) == RAW
    huge = np.full(96, 3e38, dtype=np.float32)
    huge[::5] = -1e35
    assert roundtrip(huge) == 254
    tiny = np.full(96, 3e-38, dtype=np.float32)  # the smallest binades, next to denormals
    tiny[::3] = np.float32(1.2e-38)
    tiny[1] = np.float32(5e-45)
    assert roundtrip(tiny) & 0xFF == 2
    mixed = np.random.default_rng(2).uniform(-1, 1, 768).astype(np.float32)
    mixed[100] = np.float32(2.0 ** -30)  # far below the rest: raw
    assert roundtrip(mixed) == RAW
