"""The bytes LMDB stores for a tree node (`NodeCodec`, src/node.rs:229-241), restated in plain Python: the reference the
device encoder (csrc/encode.hip) and the host one (csrc/node_codec.h) are tested against.

  split node    [2][left u32 BE][right u32 BE], then [D::Header][vector bytes] unless the node has no normal
  Descendants   [1] + the portable Roaring serialisation without run containers: u32 LE cookie 12346, u32 LE container
                count nc, nc x (u16 key = id >> 16, u16 cardinality - 1), nc x u32 byte offset of the container's body from
                the start of the serialisation, then per container, in key order, the sorted low 16 bits as u16 LE
                (cardinality <= 4096) or an 8192-byte bitmap (bit v & 7 of byte v >> 3)
"""
import struct

import numpy as np

TAG_DESCENDANTS, TAG_SPLIT = 1, 2
ROARING_COOKIE = 12346
ARRAY_MAX = 4096
BITMAP_BYTES = 8192


def split_value_len(has_normal: bool, header_size: int, vector_size: int) -> int:
    return 9 + (header_size + vector_size if has_normal else 0)


def descendants_value_bound(count: int) -> int:
    return 9 + 10 * count


def encode_split(left: int, right: int, normal: bytes | None = None) -> bytes:
    """`normal`: [D::Header][vector bytes] (the canonical form of Forest.canonical), or None for `normal: None`."""
    return bytes([TAG_SPLIT]) + struct.pack(">II", left, right) + (bytes(normal) if normal is not None else b"")


def _containers(ids: np.ndarray):
    keys = ids >> 16
    starts = np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1]))) if ids.size else np.zeros(0, np.int64)
    ends = np.append(starts[1:], ids.size)
    return [(int(keys[a]), ids[a:b] & 0xFFFF) for a, b in zip(starts, ends)]


def encode_descendants(ids) -> bytes:
    ids = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
    if ids.size > 1 and not bool(np.all(ids[1:] > ids[:-1])):
        raise ValueError("item ids must ascend strictly")
    conts = _containers(ids)
    pairs, offsets, bodies = b"", b"", []
    at = 8 + 8 * len(conts)
    for key, lows in conts:
        pairs += struct.pack("<HH", key, lows.size - 1)
        offsets += struct.pack("<I", at)
        if lows.size <= ARRAY_MAX:
            body = lows.astype("<u2").tobytes()
        else:
            bits = np.zeros(BITMAP_BYTES * 8, dtype=np.uint8)
            bits[lows] = 1
            body = np.packbits(bits, bitorder="little").tobytes()
        bodies.append(body)
        at += len(body)
    return bytes([TAG_DESCENDANTS]) + struct.pack("<II", ROARING_COOKIE, len(conts)) + pairs + offsets + b"".join(bodies)


def values_of_export(export: dict, distance, dimensions: int, node_id_of=None) -> list:
    """The value of every node slot of an `Index.export()` dict, in slot order: what Index.encode_nodes(None, node_ids=node_id_of)
    returns, restated on the CPU.  A free slot (kind 0) gives b"".  Children are written as node_id_of[child] (None: the slot
    number itself); a split node's normal is the header words of its row followed by the first vector_size bytes of the row."""
    hs, vs = distance.header_size(), distance.vector_size(dimensions)
    desc = export["descendants"]
    ident = (lambda i: int(i)) if node_id_of is None else (lambda i: int(node_id_of[int(i)]))
    out = []
    for nd in export["nodes"]:
        kind = int(nd["kind"])
        if kind == 0:
            out.append(b"")
        elif kind == 1:
            off = int(nd["offset"])
            out.append(encode_descendants(desc[off:off + int(nd["count"])]))
        elif kind == 2:
            normal = None
            if int(nd["has_normal"]):
                row = int(nd["offset"])
                hdr = np.ascontiguousarray(export["normal_headers"][row], dtype="<f4").tobytes()
                normal = hdr.ljust(hs, b"\0")[:hs] + np.ascontiguousarray(export["normal_rows"][row], dtype=np.uint8).tobytes()[:vs]
            out.append(encode_split(ident(nd["left"]), ident(nd["right"]), normal))
        else:
            raise ValueError(f"node of kind {kind}")
    return out


def decode_value(distance, dimensions: int, value: bytes):
    """("S", left, right, normal bytes or None) or ("D", ascending u32 array of item ids)."""
    value = bytes(value)
    if value[0] == TAG_SPLIT:
        left, right = struct.unpack(">II", value[1:9])
        want = distance.header_size() + distance.vector_size(dimensions)
        if len(value) == 9:
            return ("S", left, right, None)
        if len(value) != 9 + want:
            raise ValueError(f"split value of {len(value)} bytes, expected 9 or {9 + want}")
        return ("S", left, right, value[9:])
    if value[0] != TAG_DESCENDANTS:
        raise ValueError(f"unknown node tag {value[0]}")
    ser = value[1:]
    cookie, nc = struct.unpack("<II", ser[:8])
    if cookie != ROARING_COOKIE:
        raise ValueError(f"Roaring cookie {cookie}")
    out, end = [], 8 + 8 * nc
    for c in range(nc):
        key, cm1 = struct.unpack("<HH", ser[8 + 4 * c: 12 + 4 * c])
        (at,) = struct.unpack("<I", ser[8 + 4 * nc + 4 * c: 12 + 4 * nc + 4 * c])
        card = cm1 + 1
        if card <= ARRAY_MAX:
            lows = np.frombuffer(ser, dtype="<u2", count=card, offset=at).astype(np.uint32)
            end = at + 2 * card
        else:
            bits = np.unpackbits(np.frombuffer(ser, dtype=np.uint8, count=BITMAP_BYTES, offset=at), bitorder="little")
            lows = np.flatnonzero(bits).astype(np.uint32)
            if lows.size != card:
                raise ValueError(f"bitmap container of {lows.size} bits, cardinality {card}")
            end = at + BITMAP_BYTES
        out.append((np.uint32(key) << np.uint32(16)) | lows)
    if end != len(ser):
        raise ValueError(f"Descendants value of {len(value)} bytes, its containers end at {1 + end}")
    return ("D", np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32))
