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


# ---- the v0.4 - v0.6 layouts (`GenericReadNodeCodecFromV0_4_0`, src/node.rs:284-319; csrc/node_legacy.h) ------------------------
#   split node    [2][left NodeId][right NodeId][vector], NodeId = [mode u8][item u32 BE]: 11 + vector_size bytes, no header;
#                 `normal: None` is a vector `is_zero` accepts.  Leaf and Descendants values are those of v0.7.
LAYOUT_V0_7, LAYOUT_V0_5, LAYOUT_V0_4 = 0, 1, 2
LAYOUTS = {"v0.7": LAYOUT_V0_7, "v0.6": LAYOUT_V0_5, "v0.5": LAYOUT_V0_5, "v0.4": LAYOUT_V0_4}
LEGACY_SPLIT_HEAD = 11


def layout_of(layout) -> int:
    """"v0.7" | "v0.6" | "v0.5" | "v0.4" or the ah_node_layout number -> the number."""
    if isinstance(layout, str):
        if layout not in LAYOUTS:
            raise ValueError(f"unknown node layout {layout!r}: one of {sorted(LAYOUTS)}")
        return LAYOUTS[layout]
    if int(layout) not in (LAYOUT_V0_7, LAYOUT_V0_5, LAYOUT_V0_4):
        raise ValueError(f"unknown node layout {layout}")
    return int(layout)


def legacy_modes(layout) -> dict:
    """{"tree": mode byte, "item": mode byte} of a legacy layout (src/node_id.rs; v0.4: src/upgrade.rs:32-38)."""
    layout = layout_of(layout)
    if layout == LAYOUT_V0_7:
        raise ValueError("the v0.7 layout has no child modes")
    return {"tree": 1, "item": 0} if layout == LAYOUT_V0_4 else {"tree": 2, "item": 3}


def encode_split_legacy(layout, left, right, vector_bytes: bytes) -> bytes:
    """`left`, `right`: (mode, id) with mode "tree" | "item" (or the mode byte itself); the vector is never absent."""
    modes = legacy_modes(layout)
    out = bytes([TAG_SPLIT])
    for mode, ident in (left, right):
        out += struct.pack(">BI", modes[mode] if isinstance(mode, str) else int(mode), int(ident))
    return out + bytes(vector_bytes)


def vector_is_zero(distance, vector_bytes: bytes) -> bool:
    """`is_zero`: every f32 element == 0.0 (-0.0 is zero, a NaN is not; src/unaligned_vector/f32.rs:54-56), every byte of a
    binary-quantized vector 0 (binary_quantized.rs:71-73)."""
    raw = np.frombuffer(bytes(vector_bytes), dtype=np.uint8)
    if distance.binary_quantized:
        return not bool(raw.any())
    return not bool((raw.view("<u4") & np.uint32(0x7FFFFFFF)).any())


def decode_legacy_value(layout, distance, dimensions: int, value: bytes):
    """("S", (mode, left), (mode, right), vector bytes or None when is_zero accepts them) with mode "tree" | "item", or
    ("D", ascending u32 array of item ids)."""
    value = bytes(value)
    if not value or value[0] != TAG_SPLIT:
        return decode_value(distance, dimensions, value)
    modes = {v: k for k, v in legacy_modes(layout).items()}
    vs = distance.vector_size(dimensions)
    if len(value) != LEGACY_SPLIT_HEAD + vs:
        raise ValueError(f"legacy split value of {len(value)} bytes, expected {LEGACY_SPLIT_HEAD + vs}")
    lm, left, rm, right = struct.unpack(">BIBI", value[1:11])
    if lm not in modes or rm not in modes:
        raise ValueError(f"child mode bytes {lm}, {rm}: neither Tree nor Item under the layout")
    vector = value[11:]
    return ("S", (modes[lm], left), (modes[rm], right), None if vector_is_zero(distance, vector) else vector)


def _oracle_new_header(distance, dimensions: int):
    """`D::new_header` of a stored vector as header bytes, by the project's CPU oracle (the reference's summation order)."""
    from oracle import oracle as O

    def new_header(vector_bytes: bytes) -> bytes:
        v = np.frombuffer(bytes(vector_bytes), dtype=np.uint8).copy()
        h = np.zeros(2, dtype=np.float32)
        O.lib().ao_new_header(distance.metric, v.ctypes.data_as(O.C.c_void_p), dimensions, h.ctypes.data_as(O.C.c_void_p))
        return h.astype("<f4").tobytes()[:distance.header_size()]
    return new_header


def upgrade_values(layout, node_ids, values, distance, dimensions: int, new_header=None):
    """`upgrade::from_0_6_to_current` (src/upgrade.rs:183-270) on the tree values of one index, on the CPU: the split values are
    visited in key order, left child before right; every Item child becomes a new Descendants node of that one id, numbered
    last node id + 1, + 2, ... in that order; the split is rewritten in the v0.7 layout with the new ids, its normal None when
    is_zero accepts the vector and [D::new_header(vector)][vector] otherwise.  `new_header`: vector bytes -> header bytes
    (default: the CPU oracle's).  -> (new_node_ids, the v0.7 values of every node in that order, the ids that were put: the
    split nodes and the new nodes, in the order of the puts)."""
    node_ids = [int(x) for x in node_ids]
    if len(node_ids) != len(values):
        raise ValueError(f"{len(values)} values for {len(node_ids)} node ids")
    if any(b <= a for a, b in zip(node_ids, node_ids[1:])):
        raise ValueError("node ids must ascend strictly")
    if layout_of(layout) == LAYOUT_V0_7:
        return node_ids, [bytes(v) for v in values], []
    new_header = new_header or _oracle_new_header(distance, dimensions)
    last = node_ids[-1] if node_ids else 0
    out, put, new_ids, new_values = [], [], [], []
    for nid, value in zip(node_ids, values):
        dec = decode_legacy_value(layout, distance, dimensions, value)
        if dec[0] != "S":
            out.append(bytes(value))
            continue
        children = []
        for mode, ident in dec[1:3]:
            if mode == "item":
                last += 1
                new_ids.append(last)
                new_values.append(encode_descendants(np.array([ident], np.uint32)))
                put.append(last)
                ident = last
            children.append(ident)
        normal = None if dec[3] is None else new_header(dec[3]) + dec[3]
        out.append(encode_split(children[0], children[1], normal))
        put.append(nid)
    return node_ids + new_ids, out + new_values, put


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
