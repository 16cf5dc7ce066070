"""`arroy::upgrade` (src/upgrade.rs) through the device, for the tree nodes of one index: the index is opened from the old
bytes (ah_index_create_from_legacy: decoded, upgraded and linked on the device) and encoded again (ah_index_encode_nodes);
what comes back is the resident index and the `(node id, value)` puts a host writes into its `wtxn`.

The item, metadata, version and `Updated` keys of the upgrades stay host work (`MetadataCodec`, the v0.4 `updated` bitmap
exploded into keys): none of it is data-parallel.
"""
from __future__ import annotations

import numpy as np

from . import node_codec
from .dataset import Dataset, Index


def _open_and_encode(dataset: Dataset, layout, node_ids, values, roots):
    node_ids = np.ascontiguousarray(node_ids, dtype=np.uint32).ravel()
    index, _stats, legacy = Index.from_encoded(dataset, node_ids, values, roots, want_stats=True, layout=layout)
    try:
        last = int(node_ids[-1]) if node_ids.size else 0
        new_ids = last + 1 + np.arange(legacy["new_nodes"], dtype=np.int64)
        if new_ids.size and int(new_ids[-1]) > 0xFFFFFFFF:
            raise ValueError("the new node ids pass 2^32 - 1")
        id_of = np.concatenate([node_ids.astype(np.int64), new_ids]).astype(np.uint32)
        encoded = index.encode_nodes(None, node_ids=id_of) if id_of.size else []
    except Exception:
        index.close()
        raise
    return index, id_of, encoded, legacy


def from_0_6_to_current(dataset: Dataset, node_ids, values, roots):
    """`upgrade::from_0_6_to_current` (src/upgrade.rs:183-270) for the tree nodes: `node_ids` / `values` as a cursor over
    `Prefix::tree(index)` of a v0.5 / v0.6 database yields them, `roots` from its metadata.  -> (the resident index of the
    upgraded nodes, [(node id, v0.7 value)] in the order the reference puts them: per split node in key order the new
    Descendants node of its left Item child, of its right one, then the split node itself)."""
    index, id_of, encoded, legacy = _open_and_encode(dataset, "v0.6", node_ids, values, roots)
    n_old = len(encoded) - legacy["new_nodes"]
    puts, new_at = [], n_old
    for i in range(n_old):
        if encoded[i][:1] != bytes([node_codec.TAG_SPLIT]):
            continue
        modes = [values[i][1], values[i][6]]  # (the index exists: the device has accepted both mode bytes)
        for mode in modes:
            if mode == node_codec.legacy_modes("v0.6")["item"]:
                puts.append((int(id_of[new_at]), encoded[new_at]))
                new_at += 1
        puts.append((int(id_of[i]), encoded[i]))
    assert new_at == len(encoded), "the new nodes of the index are not the Item children of the values"
    return index, puts


def cosine_from_0_4_to_0_5(dataset: Dataset, node_ids, values, roots):
    """`upgrade::cosine_from_0_4_to_0_5` (src/upgrade.rs:26-146) for the tree nodes of a v0.4 database: every split value is put
    again with its children's mode bytes renumbered (Item 0 -> 3, Tree 1 -> 2), Descendants values as they are, under the same
    node ids.  The values are opened on the device first (layout "v0.4": every rule of the old layout is checked there), which
    also gives the resident index of the upgraded nodes.  -> (that index, [(node id, v0.5 value)] in key order)."""
    index, _id_of, _encoded, _legacy = _open_and_encode(dataset, "v0.4", node_ids, values, roots)
    old, new = node_codec.legacy_modes("v0.4"), node_codec.legacy_modes("v0.5")
    renumber = {old["item"]: new["item"], old["tree"]: new["tree"]}
    puts = []
    for nid, value in zip(node_ids, values):
        value = bytes(value)
        if value[:1] == bytes([node_codec.TAG_SPLIT]):
            value = value[:1] + bytes([renumber[value[1]]]) + value[2:6] + bytes([renumber[value[6]]]) + value[7:]
        puts.append((int(nid), value))
    return index, puts
