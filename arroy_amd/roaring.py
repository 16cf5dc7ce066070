"""The portable RoaringBitmap serialisation (what `RoaringBitmap::serialize_into` writes), restated in plain Python: the bytes
`Index.make_filter_roaring` / ah_filter_create_roaring accept, and the reference their expansion on the device is tested
against.  Little-endian throughout.

  u32 cookie    12346: no run containers, then u32 nc (what roaring 0.10, arroy's, writes)
                low 16 bits 12347: nc = (cookie >> 16) + 1, then ceil(nc / 8) bytes of run flags (bit i & 7 of byte i >> 3
                set: container i is a run container)
  nc x (u16 key = id >> 16, u16 cardinality - 1), keys strictly ascending
  nc x u32 byte offset of the container from the start of the serialisation: always with 12346, with 12347 only when nc >= 4
  the containers in key order, back to back:
    run       u16 n_runs, n_runs x (u16 start, u16 length - 1)
    array     cardinality <= 4096: the low 16 bits, ascending u16
    bitmap    otherwise: 8192 bytes, bit v & 63 of 64-bit word v >> 6
"""
import struct

import numpy as np

COOKIE_NO_RUNS, COOKIE_RUNS = 12346, 12347
NO_OFFSET_THRESHOLD = 4
ARRAY_MAX = 4096
BITMAP_BYTES = 8192
ARRAY, BITMAP, RUN = 0, 1, 2


def _containers(ids: np.ndarray):
    keys = ids >> 16
    starts = np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1]))) if ids.size else np.zeros(0, np.int64)
    ends = np.append(starts[1:], ids.size)
    return [(int(keys[a]), (ids[a:b] & 0xFFFF).astype(np.int64)) for a, b in zip(starts, ends)]


def runs_of(lows: np.ndarray):
    """The maximal runs of an ascending array of distinct values: (starts, lengths - 1)."""
    brk = np.flatnonzero(np.diff(lows) != 1)
    first = np.concatenate(([0], brk + 1))
    last = np.concatenate((brk, [lows.size - 1]))
    return lows[first], lows[last] - lows[first]


def array_body(lows) -> bytes:
    return np.asarray(lows).astype("<u2").tobytes()


def bitmap_body(lows) -> bytes:
    bits = np.zeros(BITMAP_BYTES * 8, dtype=np.uint8)
    bits[np.asarray(lows, dtype=np.int64)] = 1
    return np.packbits(bits, bitorder="little").tobytes()


def run_body(starts, lengths_minus_1) -> bytes:
    pairs = np.stack([np.asarray(starts), np.asarray(lengths_minus_1)], axis=1).astype("<u2") if len(starts) else np.zeros((0, 2), "<u2")
    return struct.pack("<H", len(starts)) + pairs.tobytes()


def containers(ids, runs: bool = False):
    """[(key, kind, cardinality, body bytes)] of the ascending distinct ids, as serialize() lays them out."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
    if ids.size > 1 and not bool(np.all(ids[1:] > ids[:-1])):
        raise ValueError("item ids must ascend strictly")
    out = []
    for key, lows in _containers(ids):
        body, kind = (array_body(lows), ARRAY) if lows.size <= ARRAY_MAX else (bitmap_body(lows), BITMAP)
        if runs:
            starts, lens = runs_of(lows)
            if 2 + 4 * starts.size < len(body):  # (run-encoded where that is smaller)
                body, kind = run_body(starts, lens), RUN
        out.append((key, kind, int(lows.size), body))
    return out


def assemble(conts, runs: bool = False, offsets=None) -> bytes:
    """The serialisation of [(key, kind, cardinality, body bytes)] as they are (serialize() makes them from ids; a test makes
    them by hand, malformed ones included).  runs / offsets: as serialize()."""
    nc = len(conts)
    if not runs or nc == 0:  # (12347 cannot say "no containers": its count is cookie >> 16, plus one)
        if any(kind == RUN for _, kind, _, _ in conts):
            raise ValueError("a run container under cookie 12346")
        head = struct.pack("<II", COOKIE_NO_RUNS, nc)
        with_offsets = True
    else:
        flags = bytearray((nc + 7) // 8)
        for i, (_, kind, _, _) in enumerate(conts):
            if kind == RUN:
                flags[i >> 3] |= 1 << (i & 7)
        head = struct.pack("<I", COOKIE_RUNS | ((nc - 1) << 16)) + bytes(flags)
        with_offsets = nc >= NO_OFFSET_THRESHOLD if offsets is None else bool(offsets)
    pairs = b"".join(struct.pack("<HH", key, card - 1) for key, _, card, _ in conts)
    at = len(head) + 4 * nc + (4 * nc if with_offsets else 0)
    table = b""
    for _, _, _, body in conts:
        table += struct.pack("<I", at)
        at += len(body)
    return head + pairs + (table if with_offsets else b"") + b"".join(body for _, _, _, body in conts)


def serialize(ids, runs: bool = False, offsets=None) -> bytes:
    """The serialisation of the ascending distinct `ids`.  runs=False: cookie 12346, array and bitmap containers only (equal to
    node_codec.encode_descendants(ids)[1:]).  runs=True: cookie 12347, every container run-encoded where that is smaller.
    offsets: None = the format's rule (always with 12346; with 12347 from 4 containers on); True / False force the offset
    header in or out under 12347 (a test aid: what the rule does not allow is malformed)."""
    return assemble(containers(ids, runs), runs, offsets)


def deserialize(blob) -> np.ndarray:
    """The ascending u32 ids of a serialisation; ValueError on anything the format above does not allow."""
    ser = bytes(blob)
    if len(ser) < 4:
        raise ValueError(f"{len(ser)} bytes are shorter than a cookie")
    (cookie,) = struct.unpack_from("<I", ser, 0)
    flags = None
    if cookie == COOKIE_NO_RUNS:
        if len(ser) < 8:
            raise ValueError("shorter than the headers")
        (nc,) = struct.unpack_from("<I", ser, 4)
        at = 8
    elif cookie & 0xFFFF == COOKIE_RUNS:
        nc = (cookie >> 16) + 1
        flags = ser[4:4 + (nc + 7) // 8]
        at = 4 + (nc + 7) // 8
    else:
        raise ValueError(f"Roaring cookie {cookie}")
    has_offsets = flags is None or nc >= NO_OFFSET_THRESHOLD
    pairs_at, offsets_at = at, at + 4 * nc
    pos = offsets_at + (4 * nc if has_offsets else 0)
    if pos > len(ser):
        raise ValueError("shorter than the headers")
    out, last_key = [], -1
    for c in range(nc):
        key, cm1 = struct.unpack_from("<HH", ser, pairs_at + 4 * c)
        if key <= last_key:
            raise ValueError(f"container {c}: key {key} after {last_key}")
        last_key, card = key, cm1 + 1
        if has_offsets and struct.unpack_from("<I", ser, offsets_at + 4 * c)[0] != pos:
            raise ValueError(f"container {c}: offset entry disagrees with byte {pos}")
        if flags is not None and (flags[c >> 3] >> (c & 7)) & 1:
            if pos + 2 > len(ser):
                raise ValueError(f"container {c} runs past the end")
            (n_runs,) = struct.unpack_from("<H", ser, pos)
            if pos + 2 + 4 * n_runs > len(ser):
                raise ValueError(f"container {c} runs past the end")
            pairs = np.frombuffer(ser, dtype="<u2", count=2 * n_runs, offset=pos + 2).astype(np.int64).reshape(-1, 2)
            ends = pairs[:, 0] + pairs[:, 1]
            if (ends > 0xFFFF).any() or (pairs[1:, 0] <= ends[:-1]).any():
                raise ValueError(f"container {c}: runs overlap, are out of order or reach past 65535")
            lows = np.concatenate([np.arange(a, b + 1) for a, b in zip(pairs[:, 0], ends)]) if n_runs else np.zeros(0, np.int64)
            pos += 2 + 4 * n_runs
        elif card <= ARRAY_MAX:
            if pos + 2 * card > len(ser):
                raise ValueError(f"container {c} runs past the end")
            lows = np.frombuffer(ser, dtype="<u2", count=card, offset=pos).astype(np.int64)
            if (np.diff(lows) <= 0).any():
                raise ValueError(f"container {c}: the array does not ascend strictly")
            pos += 2 * card
        else:
            if pos + BITMAP_BYTES > len(ser):
                raise ValueError(f"container {c} runs past the end")
            lows = np.flatnonzero(np.unpackbits(np.frombuffer(ser, dtype=np.uint8, count=BITMAP_BYTES, offset=pos), bitorder="little"))
            pos += BITMAP_BYTES
        if lows.size != card:
            raise ValueError(f"container {c}: {lows.size} values, cardinality {card}")
        out.append((np.uint32(key) << np.uint32(16)) | lows.astype(np.uint32))
    if pos != len(ser):
        raise ValueError(f"{len(ser)} bytes, the containers end at {pos}")
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def kinds(blob) -> dict:
    """How many containers of each kind a well-formed serialisation holds, by key: {key: kind}."""
    ser = bytes(blob)
    (cookie,) = struct.unpack_from("<I", ser, 0)
    if cookie == COOKIE_NO_RUNS:
        (nc,) = struct.unpack_from("<I", ser, 4)
        flags, at = None, 8
    else:
        nc = (cookie >> 16) + 1
        flags, at = ser[4:4 + (nc + 7) // 8], 4 + (nc + 7) // 8
    out = {}
    for c in range(nc):
        key, cm1 = struct.unpack_from("<HH", ser, at + 4 * c)
        is_run = flags is not None and (flags[c >> 3] >> (c & 7)) & 1
        out[key] = RUN if is_run else ARRAY if cm1 + 1 <= ARRAY_MAX else BITMAP
    return out
