"""Host-side mirror of arroy's public surface for the hot path: `Writer`, `ArroyBuilder`, `Reader`,
`QueryBuilder` (src/writer.rs:37-485, src/reader.rs:26-298) over an in-memory item store instead of LMDB.

Scope: this mirror exists so that the parity tests read like the reference's own tests and so that the
C ABI is exercised the way arroy's Rust host code would drive it.  It implements `Writer::build` — the full
build, and the incremental one (updated items leave the trees, new ones are routed by `ah_route_items`,
overgrown descendants are re-split by `ah_build_subtrees`, trees are added / dropped per `target_n_trees`) —
and the search; LMDB and `available_memory` batching are out of scope, the upgrades of the tree nodes are in
upgrade.py, and a `Reader` opens the tree bytes of an older data file attached with `Database.attach_stored`.  All distance / margin / split
arithmetic is done by libarroy_hip.so; the host only keeps dictionaries, a priority queue and id lists —
exactly the split of work of the Rust integration.
"""
from __future__ import annotations

import math
import random
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .dataset import Dataset, Filter, Forest
from .distances import Distance

ItemId = int


class MissingMetadata(RuntimeError):
    """arroy::Error::MissingMetadata(index) (src/error.rs:48-49)."""

    def __init__(self, index: int):
        super().__init__(f"Metadata are missing on index {index}, You must build your database before attempting "
                         "to read it")
        self.index = index


class NeedBuild(RuntimeError):
    """arroy::Error::NeedBuild(index) (src/error.rs:51-52)."""

    def __init__(self, index: int):
        super().__init__(f"The trees have not been built after an update on index {index}")
        self.index = index


class UnmatchingDistance(RuntimeError):
    """arroy::Error::UnmatchingDistance { expected, received } (src/error.rs:34-41)."""

    def __init__(self, expected: str, received: str):
        super().__init__(f"Invalid distance provided. Got {received} but expected {expected}")
        self.expected, self.received = expected, received


class InvalidVecDimension(_lib.InvalidVecDimension):
    """arroy::Error::InvalidVecDimension { expected, received } (src/error.rs:17-23)."""

    def __init__(self, expected: int, received: int):
        _lib.ArroyHipError.__init__(self, 1, f"Invalid vector dimensions. Got {received} but expected {expected}")
        self.expected, self.received = expected, received

    def __str__(self) -> str:
        return self.message


def target_n_trees(n_trees: Optional[int], dimensions: int, n_items: int, n_roots: int) -> int:
    """`target_n_trees` (src/writer.rs:1358-1394): explicit option, else the fitted formula, with the
    "do not shrink by less than 20 %" rule."""
    if n_trees is not None:
        return int(n_trees)
    nb_vec = float(n_items)
    if nb_vec < 10_000.0:
        nb = 2.0 ** (math.log2(nb_vec) - 6.0) if nb_vec > 0 else 0.0
    else:
        nb = 2.0 ** (math.log10(nb_vec) + math.log10(float(dimensions)) + (768.0 / float(dimensions)) ** 4.0)
    nb_trees = int(math.ceil(nb))
    if n_roots > nb_trees:
        to_remove = n_roots - nb_trees
        if nb_trees == 0 or (to_remove / nb_trees) < 0.20:
            nb_trees = n_roots
    return nb_trees


def roots_after_drop(roots: Sequence[int], n_drop: int) -> Tuple[List[int], List[int]]:
    """`delete_extra_trees` (src/writer.rs:631-655) on the roots alone: `n_drop` times `roots.swap_remove(0)`, stopping when
    the roots run out.  Returns (the roots that stay, in the order the swap_removes leave them; the dropped roots, in the order
    they were dropped).  From [r0 .. r5] and 4: ([r2, r1], [r0, r5, r4, r3])."""
    kept, dropped = list(roots), []
    for _ in range(max(0, int(n_drop))):
        if not kept:
            break
        dropped.append(kept[0])
        kept[0] = kept[-1]
        kept.pop()
    return kept, dropped


class TreeStore:
    """Host-side tree nodes — what arroy keeps in LMDB under `Key::tree` (src/node.rs:216-241):
    id -> ("D", ascending ids) | ("S", left, right, header f32[], vector bytes or None)."""

    def __init__(self):
        self.nodes: Dict[int, tuple] = {}
        self.roots: List[int] = []
        self._next = 0
        self._available: List[int] = []
        self.last_import: Dict[int, int] = {}  # import_tree: forest node -> store id of the tree it imported last

    def begin_build(self) -> None:
        """`ConcurrentNodeIds::new(used_tree_node)` (src/parallel.rs:222-237, src/writer.rs:516-518): taken BEFORE the
        build deletes anything — ids freed by earlier builds are handed out first (ascending), ids freed by this
        build only become available to the next one."""
        self._next = max(self.nodes) + 1 if self.nodes else 0
        self._available = [i for i in range(self._next) if i not in self.nodes]

    def next_id(self) -> int:  # ConcurrentNodeIds::next (src/parallel.rs:239-254)
        if self._available:
            return self._available.pop(0)
        self._next += 1
        return self._next - 1

    def delete_tree(self, node: int) -> None:  # src/writer.rs:1263-1277
        for nid in self.subtree_ids(node):
            del self.nodes[nid]

    def delete_items(self, node: int, to_delete: set, split_after: int):
        """`delete_items_in_file` (src/writer.rs:1021-1114): remove `to_delete` below `node`; a split whose child
        became empty is replaced by the other child, two descendants that fit together are merged into their parent.
        Returns (new node id, ids of the branch if it is a single Descendants node else None)."""
        nd = self.nodes[node]
        if nd[0] == "D":
            kept = np.array([i for i in nd[1] if int(i) not in to_delete], dtype=np.uint32)
            if len(kept) != len(nd[1]):
                self.nodes[node] = ("D", kept)
            return node, kept
        _, left, right, hdr, vec = nd
        new_left, left_items = self.delete_items(left, to_delete, split_after)
        new_right, right_items = self.delete_items(right, to_delete, split_after)
        if left_items is not None and len(left_items) == 0:
            self.nodes.pop(new_left, None)
            self.nodes.pop(node, None)
            return new_right, right_items
        if right_items is not None and len(right_items) == 0:
            self.nodes.pop(new_right, None)
            self.nodes.pop(node, None)
            return new_left, left_items
        if left_items is not None and right_items is not None and len(left_items) + len(right_items) <= split_after:
            total = np.union1d(left_items, right_items).astype(np.uint32)
            self.nodes.pop(new_left, None)
            self.nodes.pop(new_right, None)
            self.nodes[node] = ("D", total)
            return node, total
        if new_left != left or new_right != right:
            self.nodes[node] = ("S", new_left, new_right, hdr, vec)
        return node, None

    def apply_delta(self, delta: dict, dense: Dict[int, int]) -> None:
        """What Index.delete_items did to the resident index, done to this store: `delta` speaks in the dense node indices of
        the view the index was made from, `dense` (store id -> index, `to_view`'s keep[4]) maps them back.  A node that
        became a Descendants node loses its plane; a split node keeps its own."""
        back = {i: nid for nid, i in dense.items()}
        for i in delta["removed"]:
            del self.nodes[back[int(i)]]
        desc = delta["desc"]
        for i, nd in zip(delta["put_index"], delta["put"]):
            nid = back[int(i)]
            if int(nd["kind"]) == 1:
                off, cnt = int(nd["offset"]), int(nd["count"])
                self.nodes[nid] = ("D", np.array(desc[off:off + cnt], dtype=np.uint32))
            else:
                old = self.nodes[nid]
                self.nodes[nid] = ("S", back[int(nd["left"])], back[int(nd["right"])], old[3], old[4])
        self.roots = [back[int(r)] for r in delta["roots"]]

    def import_tree(self, forest: Forest, tree: int, root_id: Optional[int] = None) -> int:
        """Copy tree `tree` of a freshly built ah_forest; children get fresh ids before their parent (the order
        `make_tree_in_file` allocates them, src/writer.rs:1235-1258), the root takes `root_id` when given
        (`Some(descendant_id)`, src/writer.rs:693-702)."""
        order, stack = [], [int(forest.roots[tree])]
        while stack:  # reverse post-order, then reversed: children before parents
            i = stack.pop()
            order.append(i)
            nd = forest.nodes[i]
            if nd["kind"] == 2:
                stack += [int(nd["left"]), int(nd["right"])]
        ids: Dict[int, int] = {}
        for i in reversed(order):
            nd = forest.nodes[i]
            is_root = i == int(forest.roots[tree])
            ids[i] = root_id if (is_root and root_id is not None) else self.next_id()
            if nd["kind"] == 1:
                self.nodes[ids[i]] = ("D", forest.descendants_of(i).copy())
            else:
                normal = forest.normal_of(i)
                hdr, vec = normal if normal is not None else (np.zeros(forest.distance.header_size() // 4, np.float32), None)
                self.nodes[ids[i]] = ("S", ids[int(nd["left"])], ids[int(nd["right"])], hdr,
                                      None if vec is None else vec.tobytes())
        self.last_import = ids
        return ids[int(forest.roots[tree])]

    def import_streamed_tree(self, streamed, tree: int, root_id: Optional[int] = None) -> int:
        """import_tree for a tree of a StreamedForest (what a streaming / device-group build delivered): the same node
        order, hence the same ids as importing the ah_forest of a single-device build."""
        root = int(streamed.roots[tree])
        order, stack = [], [root]
        while stack:
            i = stack.pop()
            order.append(i)
            if i in streamed.splits:
                stack += [streamed.splits[i][1], streamed.splits[i][2]]
        hs = streamed.distance.header_size()
        ids: Dict[int, int] = {}
        for i in reversed(order):
            ids[i] = root_id if (i == root and root_id is not None) else self.next_id()
            if i in streamed.leaves:
                self.nodes[ids[i]] = ("D", np.array(streamed.leaves[i][0], dtype=np.uint32))
            else:
                nb, left, right = streamed.splits[i][:3]
                hdr = np.frombuffer(nb[:hs], dtype=np.float32).copy() if nb is not None else np.zeros(hs // 4, np.float32)
                self.nodes[ids[i]] = ("S", ids[left], ids[right], hdr, None if nb is None else bytes(nb[hs:]))
        return ids[root]

    def subtree_ids(self, root: int) -> List[int]:
        out, stack = [], [root]
        while stack:
            i = stack.pop()
            out.append(i)
            nd = self.nodes[i]
            if nd[0] == "S":
                stack += [nd[1], nd[2]]
        return out

    def to_view(self, distance: type[Distance], dimensions: int):
        """Dense arrays in the ah_forest_view shape (records [header][vector]); returns (view, keepalive)."""
        import ctypes as C
        order = sorted(self.nodes)
        dense = {nid: i for i, nid in enumerate(order)}
        hs, vs = distance.header_size(), distance.vector_size(dimensions)
        node_dt = np.dtype([("kind", "u1"), ("has_normal", "u1"), ("reserved", "<u2"), ("tree", "<u4"), ("left", "<u4"),
                            ("right", "<u4"), ("offset", "<u8"), ("count", "<u4"), ("depth", "<u4")], align=True)
        nodes = np.zeros(len(order), dtype=node_dt)
        normals, desc = bytearray(), []
        n_desc = 0
        for nid in order:
            nd, i = self.nodes[nid], dense[nid]
            if nd[0] == "D":
                nodes[i] = (1, 0, 0, 0, 0, 0, n_desc, len(nd[1]), 0)
                desc.append(np.asarray(nd[1], dtype=np.uint32))
                n_desc += len(nd[1])
            else:
                has = nd[4] is not None
                nodes[i] = (2, 1 if has else 0, 0, 0, dense[nd[1]], dense[nd[2]], len(normals), 0, 0)
                if has:
                    normals += np.asarray(nd[3], dtype=np.float32).tobytes().ljust(hs, b"\0")[:hs] + nd[4]
        normals_a = np.frombuffer(bytes(normals), dtype=np.uint8).copy() if normals else np.zeros(1, np.uint8)
        desc_a = np.concatenate(desc).astype(np.uint32) if desc and n_desc else np.zeros(1, np.uint32)
        roots_a = np.array([dense[r] for r in self.roots], dtype=np.uint32) if self.roots else np.zeros(1, np.uint32)
        v = _lib.AhForestView()
        v.n_trees, v.n_nodes = len(self.roots), len(order)
        v.roots = roots_a.ctypes.data_as(C.POINTER(C.c_uint32))
        v.nodes = C.cast(nodes.ctypes.data, C.POINTER(_lib.AhNode))
        v.normals = normals_a.ctypes.data_as(C.POINTER(C.c_uint8))
        v.normals_len = len(normals)
        v.normal_stride, v.normal_vector_offset, v.normal_header_offset = hs + vs, hs, 0
        v.descendants = desc_a.ctypes.data_as(C.POINTER(C.c_uint32))
        v.descendants_len = n_desc
        return v, (nodes, normals_a, desc_a, roots_a, dense)

    def stats(self, root: int) -> dict:  # `Reader::stats` per tree (src/reader.rs:210-252)
        depth = splits = dummies = descs = 0
        stack = [(root, 1)]
        while stack:
            i, d = stack.pop()
            depth = max(depth, d)
            nd = self.nodes[i]
            if nd[0] == "D":
                descs += 1
            else:
                splits += 1
                dummies += 0 if nd[4] is not None else 1
                stack += [(nd[1], d + 1), (nd[2], d + 1)]
        return {"depth": depth, "split_nodes": splits, "dummy_normals": dummies, "descendants": descs}


class _IndexState:
    def __init__(self):
        self.items: Dict[ItemId, np.ndarray] = {}
        self.updated: set = set()          # the `Updated` key set (src/writer.rs:391)
        self.metadata: Optional[dict] = None
        self.dataset: Optional[Dataset] = None
        self.trees: Optional[TreeStore] = None
        self.index = None    # arroy_amd.Index: dataset + tree nodes resident in HBM
        self._keep = None    # arrays the index view was built from
        self.stored_trees = None  # (node ids, values): the tree bytes of an attached data file (Database.attach_stored)
        self.device_deletes = 0  # builds that took the updated items out of the trees on the device (Index.delete_items)
        self.device_inserts = 0  # builds that ended with the resident index still serving (Index.insert_items / graft)
        self.index_uploads = 0   # indexes made from a whole view of the store (every node, id and normal uploaded)
        self.device_compactions = 0  # builds that ended with a compaction of the resident index (Index.compact)
        self.device_drops = 0    # builds that dropped their extra trees on the resident index (Index.drop_trees)
        # nodes whose values a build that kept its resident index encoded on the device for ArroyBuilder.encoded_store
        # (Index.encode_nodes of the nodes its deltas put and its grafts added, not of the whole index)
        self.device_encoded_nodes = 0


def compaction_due(fp: dict) -> bool:
    """Whether a resident index with this footprint (Index.footprint) is compacted at the end of a build: more dead normal rows
    than live ones, more free node slots than nodes in use, or room for more than twice the live rows.  The 1x threshold bounds
    the normals at twice a fresh index's (apart from the graft's own geometric head-room) and makes the work amortised O(1): a
    compaction copies `live` rows only after at least `live` rows have died, each of which was uploaded once over a link far
    slower than HBM.  Derived, not measured."""
    live = fp["live_normals"]
    in_use = fp["n_nodes"] - fp["free_slots"]
    return fp["n_normals"] - live > live or fp["free_slots"] > in_use or fp["normals_cap"] > 2 * max(1, live)


class Database:
    """Stand-in for `Database<D>` (src/lib.rs:156) + its LMDB environment: one item store per index."""

    def __init__(self, distance: type[Distance]):
        self.distance = distance
        self._indexes: Dict[int, _IndexState] = {}

    def remap_data_type(self, distance: type[Distance]) -> "Database":
        """`database.remap_data_type::<NodeCodec<D2>>()`: the same store seen through another distance type."""
        other = Database(distance)
        other._indexes = self._indexes
        return other

    def _state(self, index: int) -> _IndexState:
        return self._indexes.setdefault(index, _IndexState())

    def attach_stored(self, index: int, dataset: Dataset, items: Dict[ItemId, np.ndarray], roots: Sequence[int], node_ids, values) -> None:
        """An index as an existing data file holds it: `dataset` has the items staged, `roots` are those of the metadata, and
        `node_ids` / `values` are the tree keys and their bytes as a cursor yields them, of whatever version wrote the file.
        Nothing is decoded here: `Reader.open(database, index, version)` opens the resident index from the bytes."""
        st = self._state(index)
        st.items = {int(i): np.ascontiguousarray(v, dtype=np.float32) for i, v in items.items()}
        st.updated = set()
        st.dataset, st.trees, st.index = dataset, None, None
        st.stored_trees = ([int(i) for i in node_ids], list(values))
        st.metadata = {"dimensions": dataset.dimensions, "items": sorted(st.items), "roots": [int(r) for r in roots],
                       "distance": self.distance.name}


class Writer:
    """`Writer<D>` (src/writer.rs:271-485)."""

    def __init__(self, database: Database, index: int, dimensions: int):
        self.database, self.index, self.dimensions = database, index, int(dimensions)
        self._st = database._state(index)

    def add_item(self, item: ItemId, vector: Sequence[float]) -> None:  # src/writer.rs:380-394
        v = np.ascontiguousarray(vector, dtype=np.float32).ravel()
        if v.size != self.dimensions:
            raise InvalidVecDimension(self.dimensions, v.size)
        self._st.items[int(item)] = v.copy()
        self._st.updated.add(int(item))

    append_item = add_item  # same observable effect without an LMDB cursor (src/writer.rs:396-432)

    def del_item(self, item: ItemId) -> bool:  # src/writer.rs:434-443
        if int(item) in self._st.items:
            del self._st.items[int(item)]
            self._st.updated.add(int(item))
            return True
        return False

    def clear(self) -> None:  # src/writer.rs:445-470
        self._st.__init__()

    def is_empty(self) -> bool:
        return not self._st.items

    def contains_item(self, item: ItemId) -> bool:
        return int(item) in self._st.items

    def need_build(self) -> bool:  # src/writer.rs:355-363
        return bool(self._st.updated) or self._st.metadata is None

    def builder(self, rng: Optional[random.Random] = None, devices: Optional[Sequence[int]] = None) -> "ArroyBuilder":
        return ArroyBuilder(self, rng if rng is not None else random.Random(), devices=devices)


class ArroyBuilder:
    """`ArroyBuilder` (src/writer.rs:37-265): n_trees / split_after / cancel / progress / build."""

    def __init__(self, writer: Writer, rng: random.Random, devices: Optional[Sequence[int]] = None):
        """`devices`: stage the items on every listed device (a DatasetGroup: one host pass) and build the new trees on all
        of them, tree t on device t mod len(devices) — the same forest as one device.  None: one device (device 0)."""
        self._w, self._rng = writer, rng
        self._devices = None if devices is None else [int(d) for d in devices]
        if self._devices is not None and not self._devices:
            raise ValueError("devices must list at least one device")
        self._group = None
        self._n_trees: Optional[int] = None
        self._split_after: Optional[int] = None
        self._cancel: Optional[Callable[[], bool]] = None
        self._progress: Optional[Callable] = None
        self.device_delete = True  # False: the removal of updated items always on the host (what the tests compare with)
        # False: the index that serves the searches after an incremental build is always made from a view of the whole store
        self.device_insert = True
        # False: the resident index keeps its free node slots and orphaned normal rows whatever they amount to
        self.device_compact = True
        # True: the index that serves the searches is audited on the device at the end of build() (Index.audit: validity
        # and the per-tree stats against the store's); a finding raises AssertionError
        self.device_audit = False
        # True: a build that drops trees keeps its resident index and drops them there (Index.drop_trees) instead of closing
        # it and uploading an index from the whole view.  OFF by default: tests/test_gpu_index_insert.py
        # (test_writer_keeps_the_index_and_builds_the_same_trees) pins the fall-back counts of a tree-dropping build, so the
        # default can only flip in a change that may touch that test
        self.device_drop = False
        # True: the forests of this build stay on the device (Dataset.build_forest / build_subtrees with resident=True) and the
        # index is made or extended from them there (Index.from_forest, Index.graft_forest) — the first full build makes its
        # index in the store's numbering, slices after the first and the sub-trees of an incremental build are grafted — so no
        # index is uploaded from a whole view (index_uploads stays).  OFF by default, like device_drop
        self.device_forest = False
        # True: a build that keeps its resident index suspends the index's live filters (Filter.suspend) instead of closing
        # them, and leaves them suspended for the caller to resume with its delta (Index.resume_filters); the compaction at
        # the end of the build is then no longer skipped on their account
        self.keep_filters = False
        # A dict: build() keeps it equal to {node id: `NodeCodec` value} of the TreeStore — what the tree keys of LMDB would
        # hold — written only from device encodes (Index.encode_nodes).  A build whose resident index has followed the store
        # removes the ids its deltas removed and encodes only the nodes the deltas put and the grafts added; any other build
        # replaces the content with the encoding of every node of the new index.  None: nothing is encoded
        self.encoded_store: Optional[dict] = None
        self._enc_removed: set = set()  # store ids the deltas of this build removed ...
        self._enc_put: set = set()      # ... and the ones they put or a graft added

    def _note_delta(self, delta: dict, dense: Dict[int, int], back: Optional[Dict[int, int]] = None) -> None:
        """What a delta of the resident index means for encoded_store, in store ids (before TreeStore.apply_delta).  `back`:
        the inverse of `dense` where the caller has it already."""
        if self.encoded_store is None:
            return
        if back is None:
            back = {i: nid for nid, i in dense.items()}
        self._enc_removed.update(back[int(i)] for i in delta["removed"])
        self._enc_put.update(back[int(i)] for i in delta["put_index"])

    def _mirror_encoded(self, st: "_IndexState", followed: bool) -> None:
        """encoded_store after a build: see __init__."""
        store = self.encoded_store
        if store is None:
            return
        if st.index is None:
            store.clear()
            return
        dense = st._keep[4]  # store id -> node slot of the index, after any compaction
        id_of = np.zeros(st.index.export_info()["n_nodes"], dtype=np.uint32)
        for nid, i in dense.items():
            id_of[i] = nid
        if followed:
            for nid in self._enc_removed:
                store.pop(nid, None)
            put = sorted(nid for nid in self._enc_put if nid in st.trees.nodes)
            values = st.index.encode_nodes(np.array([dense[nid] for nid in put], dtype=np.uint32), node_ids=id_of)
            store.update(zip(put, values))
            st.device_encoded_nodes += len(put)
        else:
            order = sorted(dense, key=dense.get)
            values = st.index.encode_nodes(np.array([dense[nid] for nid in order], dtype=np.uint32), node_ids=id_of)
            store.clear()
            store.update(zip(order, values))

    def n_trees(self, n: int) -> "ArroyBuilder":
        self._n_trees = int(n)
        return self

    def split_after(self, n: int) -> "ArroyBuilder":
        self._split_after = int(n)
        return self

    def available_memory(self, _bytes: int) -> "ArroyBuilder":
        return self  # HBM-resident build: the page-budgeted batching of src/writer.rs:685-723 does not apply

    def cancel(self, fn: Callable[[], bool]) -> "ArroyBuilder":
        self._cancel = fn
        return self

    def progress(self, fn: Callable) -> "ArroyBuilder":
        self._progress = fn
        return self

    def build(self) -> None:
        """`Writer::build` (src/writer.rs:487-629): a full build when the index has no trees yet, otherwise the
        incremental path — remove updated items from the trees (:525), route the new / changed ones through the
        existing planes (:541-542, `ah_route_items`), re-split the descendants that outgrew `split_after` (:660-739,
        `ah_build_subtrees`), then add or drop whole trees to reach `target_n_trees` (:521-524, 556-561)."""
        w, st = self._w, self._w._st
        if self._cancel is not None and self._cancel():
            raise _lib.BuildCancelled(2, "build cancelled")
        dist = w.database.distance
        ids = np.array(sorted(st.items), dtype=np.uint32)
        n = ids.size
        split_after = self._split_after or w.dimensions
        # The index of the last build stays for this build's delete and routing (suspended while the dataset is updated)
        # when this will be an incremental build on the same dataset that drops no tree, or drops them on the index
        # (device_drop): `delete_extra_trees` runs before the removal, and without Index.drop_trees the resident index would
        # still hold the dropped trees.
        resident = st.index
        st.index = None
        followed = False
        self._enc_removed, self._enc_put = set(), set()
        keep = (resident is not None and self.device_delete and n > split_after and st.trees is not None
                and bool(st.trees.roots) and st.metadata is not None
                and (self.device_drop
                     or target_n_trees(self._n_trees, w.dimensions, n, len(st.trees.roots)) >= len(st.trees.roots)))
        try:  # (whatever happens in between, the kept index does not linger suspended with its normals in HBM)
            if resident is not None:
                if keep:
                    resident.suspend(keep_filters=self.keep_filters)
                else:
                    resident.close()  # (an update of the dataset refuses while an index holds it)
                    resident = None
            self._group = None
            ds = self._update_dataset(st) if n else None  # the last build's dataset with this build's item changes, if any
            if resident is not None:
                if ds is not None:
                    resident.resume(ds)
                else:  # staged afresh: the index is of the old dataset
                    resident.close()
                    resident = None
            if ds is None and n and self._devices is not None:
                from .dataset import DatasetGroup
                vecs = np.stack([st.items[int(i)] for i in ids])
                self._group = DatasetGroup(dist, w.dimensions, n, self._devices)
                self._group.upload_vectors(ids, vecs)
                if dist.metric == 3:
                    self._group.preprocess_dot()
                self._group.finalize()
                ds = self._group.member(0)  # search and the incremental paths use member 0 (it keeps the group alive)
            elif ds is None and n:
                vecs = np.stack([st.items[int(i)] for i in ids])
                ds = Dataset(dist, w.dimensions, n)
                ds.upload_vectors(ids, vecs)
                if dist.metric == 3:
                    ds.preprocess_dot()  # pre_process_items, src/writer.rs:964-976
                ds.finalize()
            st.dataset = ds
            if n <= split_after:
                # clear_db_and_create_a_single_leaf (src/writer.rs:916-962): ONE Descendants root, whatever n_trees says
                st.trees = TreeStore()
                if n:
                    root = st.trees.next_id()
                    st.trees.nodes[root] = ("D", ids.copy())
                    st.trees.roots = [root]
            elif st.trees is None or not st.trees.roots or st.metadata is None:
                st.trees = TreeStore()
                n_trees = target_n_trees(self._n_trees, w.dimensions, n, 0)
                made = self._add_trees_on_device(ds, st.trees, n_trees, split_after) if self.device_forest and self._group is None else None
                if made is not None:
                    st.index, st._keep = made
                elif not st.trees.roots:
                    self._add_trees(ds, st.trees, n_trees, split_after)
            else:
                kept = self._incremental(ds, st, ids, split_after, resident)
                if kept is not None:  # the resident index has followed the store: it serves the searches from here on
                    st.index, st._keep, resident = resident, kept, None
                    st.device_inserts += 1
                    followed = True
        finally:
            if resident is not None:
                resident.close()  # (a second close is a no-op: _incremental closes it when it is done with it)
        if n and st.index is None:
            view, keep = st.trees.to_view(dist, w.dimensions)
            from .dataset import Index
            st.index, st._keep = Index(ds, None, view=view), keep
            st.index_uploads += 1
        self._mirror_encoded(st, followed)
        if self.device_audit and st.index is not None:
            _assert_audit(st.index.audit(trees=True), st.trees)
        st.metadata = {"dimensions": w.dimensions, "items": [int(i) for i in ids], "roots": list(st.trees.roots),
                       "distance": dist.name}  # src/writer.rs:611-626
        st.updated.clear()

    def _update_dataset(self, st: "_IndexState") -> Optional[Dataset]:
        """The dataset (or device group) of the last build with this build's item changes applied (Dataset.update_vectors):
        remove = updated, upsert = updated & items (src/writer.rs:497-505), so only the changed rows are staged.  None when
        there is nothing to update — the first build, after `clear()`, another distance / dimension / device list — or
        when the library refuses the update (e.g. another index on the dataset is still alive): the caller stages afresh."""
        w, prev = self._w, st.dataset
        dist = w.database.distance
        if prev is None or not prev._h or prev.distance is not dist or prev.dimensions != w.dimensions:
            return None
        group = prev._owner
        if (group is None) != (self._devices is None) or (group is not None and group.devices != self._devices):
            return None
        remove = np.array(sorted(st.updated), dtype=np.uint32)
        upsert = np.array([i for i in remove if int(i) in st.items], dtype=np.uint32)
        vecs = np.stack([st.items[int(i)] for i in upsert]) if upsert.size else np.zeros((0, w.dimensions), np.float32)
        target = group if group is not None else prev
        try:
            target.update_vectors(remove, upsert, vecs)
        except _lib.ArroyHipError:
            return None
        if dist.metric == 3:
            target.preprocess_dot()  # pre_process_items, src/writer.rs:964-976
        self._group = group
        return prev

    def _seeds(self, count: int) -> List[int]:
        return [self._rng.getrandbits(64) for _ in range(count)]  # one RNG per task (src/writer.rs:575,795)

    def _add_trees(self, ds: Dataset, trees: TreeStore, count: int, split_after: int, grafted=None, resident: bool = False) -> None:
        """`grafted(forest, maps)`: called after the trees of every forest are in the store, with the forest node -> store id
        map of each of its trees (the one-device path only)."""
        if count <= 0:
            return
        # arroy's formula (src/writer.rs:1371-1380) explodes for >= 10 000 items of fewer than 768 dimensions
        # ((768 / dims)^4 in the exponent); the reference then builds that many trees, and so does this mirror
        # (ah_node.tree is 32 bits since ABI v2) — in slices, so that the host-side forest stays bounded.
        seeds = self._seeds(count)
        if self._group is not None:
            self._add_trees_group(trees, seeds, split_after)
            return
        for lo in range(0, count, 4096):
            forest = ds.build_forest(seeds[lo:lo + 4096], split_after=split_after, cancel=self._cancel,
                                     progress=self._progress, resident=resident)
            maps = []
            try:
                for t in range(forest.n_trees):
                    root = trees.next_id()  # roots are allocated before their subtree (src/writer.rs:556-561)
                    trees.import_tree(forest, t, root_id=root)
                    trees.roots.append(root)
                    maps.append(trees.last_import)
                if grafted is not None:
                    grafted(forest, maps)
            finally:
                forest.close()

    def _add_trees_on_device(self, ds: Dataset, trees: TreeStore, count: int, split_after: int):
        """_add_trees of a full build with device_forest: every slice is built resident; the first becomes the index in the
        store's numbering (Index.from_forest), the others are grafted as new roots (Index.graft_forest).  -> (index, _keep), or
        None when the library refused a step: the trees are in the store all the same and the caller makes the index from its view."""
        from .dataset import Index
        state = {"ix": None, "dense": None, "ok": True}

        def grafted(forest, maps):
            if not state["ok"]:
                return
            new_dense = {nid: i for i, nid in enumerate(sorted(trees.nodes))}
            new_index = np.zeros(len(forest.nodes), dtype=np.uint32)
            for ids_of in maps:
                for k, nid in ids_of.items():
                    new_index[k] = new_dense[nid]
            try:
                if state["ix"] is None:
                    state["ix"] = Index.from_forest(ds, forest, new_index)
                else:
                    state["ix"].graft_forest(forest, np.full(len(maps), _lib.NEW_ROOT, dtype=np.uint32), new_index)
                state["dense"] = new_dense
            except _lib.ArroyHipError:
                state["ok"] = False
        try:
            self._add_trees(ds, trees, count, split_after, grafted=grafted, resident=True)
        except BaseException:
            if state["ix"] is not None:
                state["ix"].close()
            raise
        if not state["ok"] or state["ix"] is None:
            if state["ix"] is not None:
                state["ix"].close()
            return None
        return state["ix"], (None, None, None, None, {nid: state["dense"][nid] for nid in trees.nodes})

    def _add_trees_group(self, trees: TreeStore, seeds: List[int], split_after: int) -> None:
        """_add_trees on the device group: one streamed build over all members, imported tree by tree in tree order."""
        import threading
        cflag, watcher_stop = None, None
        if self._cancel is not None:
            import ctypes
            cflag, watcher_stop = ctypes.c_int(0), threading.Event()
            cancel = self._cancel

            def _watch():
                while not watcher_stop.wait(0.0005):
                    if cancel():
                        cflag.value = 1
                        return
            threading.Thread(target=_watch, daemon=True).start()
        try:
            for lo in range(0, len(seeds), 4096):
                _roots, _stats, _per, streamed = self._group.build_stream(
                    seeds[lo:lo + 4096], split_after=split_after, cancel=cflag, progress=self._progress)
                for t in range(len(streamed.roots)):
                    root = trees.next_id()
                    trees.import_streamed_tree(streamed, t, root_id=root)
                    trees.roots.append(root)
        finally:
            if watcher_stop is not None:
                watcher_stop.set()

    def _incremental(self, ds: Dataset, st: "_IndexState", ids: np.ndarray, split_after: int, resident=None):
        """`resident`: the last build's Index, resumed on the updated dataset (build() has checked that no tree is dropped, or
        that device_drop is on): the dropped trees, the removal and the routing run on it.  None: the removal on the host, the
        routing on a throw-away index of the store's view.  Returns the new `_keep` when `resident` has followed every step and is the index of the store as it is now
        (device_insert); None when it has been closed here and the caller makes an index from the view."""
        from .dataset import Index
        w, trees, dist = self._w, st.trees, self._w.database.distance
        present = set(int(i) for i in ids)
        to_delete = np.array(sorted(st.updated), dtype=np.uint32)                 # :504
        to_insert = np.array(sorted(i for i in st.updated if i in present), dtype=np.uint32)  # :505
        import sys
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 100000))
        trees.begin_build()  # node ids in use are snapshotted before anything is deleted (:516-518)
        # target_n_trees / delete_extra_trees (:521-522, 631-655): the oldest tree first, `roots.swap_remove(0)`
        want = target_n_trees(self._n_trees, w.dimensions, len(ids), len(trees.roots))
        n_drop = max(0, len(trees.roots) - want)
        if n_drop and resident is not None:
            # on the resident index (build() keeps it for a tree-dropping build only with device_drop); the roots come back
            # sorted when no delete, which sorts them itself, follows.  A failure leaves the index unchanged: it is closed and
            # the build goes on on the host path, as after a failed insert
            try:
                delta = resident.drop_trees(n_drop, sort_roots=not to_delete.size)
                self._note_delta(delta, st._keep[4])
                trees.apply_delta(delta, st._keep[4])
                st.device_drops += 1
                n_drop = 0
            except _lib.ArroyHipError:
                resident.close()
                resident = None
        if n_drop:
            trees.roots, dropped = roots_after_drop(trees.roots, n_drop)
            for root in dropped:
                trees.delete_tree(root)
        # delete_items_from_trees (:525, 979-1114): updated ids leave the trees, emptied / shrunken branches collapse
        if resident is not None:
            try:
                dense = st._keep[4]
                if to_delete.size:
                    delta = resident.delete_items(to_delete, split_after)
                    self._note_delta(delta, dense)
                    trees.apply_delta(delta, dense)
                    st.device_deletes += 1
            except BaseException:
                resident.close()
                raise
        elif to_delete.size:
            gone = set(int(i) for i in to_delete)
            trees.roots = [trees.delete_items(root, gone, split_after)[0] for root in trees.roots]
        trees.roots.sort()
        # insert_items_in_current_trees (:541-542): one call for all trees.  On the device path (Index.insert_items) the
        # resident index takes the ids into its lists itself and then follows the store through every later step
        # (Index.graft), so that it serves the searches after this build; any failure of that path leaves the host path,
        # which ends with an index made from the view.
        follow = resident is not None and self.device_insert
        grown: Dict[int, List[int]] = {}
        if to_insert.size and trees.roots:
            if resident is None:
                view, keep = trees.to_view(dist, w.dimensions)
                dense = keep[4]
                resident = Index(ds, None, view=view)
            back = {i: nid for nid, i in dense.items()}
            seeds = self._seeds(len(trees.roots))
            delta = None
            if follow:
                try:
                    delta = resident.insert_items(to_insert, seeds)
                except _lib.ArroyHipError:
                    follow = False
            if delta is not None:
                self._note_delta(delta, dense, back)
                trees.apply_delta(delta, dense)
                grown = {back[int(i)]: [] for i in delta["put_index"]}
            else:
                try:
                    leaf_of = resident.route_items(to_insert, seeds)
                finally:
                    resident.close()
                    resident = None
                for t in range(leaf_of.shape[0]):
                    for i, leaf in enumerate(leaf_of[t]):
                        grown.setdefault(back[int(leaf)], []).append(int(to_insert[i]))
                for nid, extra in grown.items():
                    trees.nodes[nid] = ("D", np.union1d(trees.nodes[nid][1], np.array(extra, dtype=np.uint32)).astype(np.uint32))
        follow = follow and resident is not None
        state = {"dense": dense if follow else None, "ok": follow}

        def graft(forest, maps, targets):
            """The trees of `forest`, imported with `maps`, join the resident index; its numbering becomes the store's."""
            if not state["ok"]:
                return
            new_dense = {nid: i for i, nid in enumerate(sorted(trees.nodes))}
            new_index = np.full(len(forest.nodes), 0xFFFFFFFF, dtype=np.uint32)
            tg = np.full(len(maps), _lib.NEW_ROOT, dtype=np.uint32)
            for t, ids_of in enumerate(maps):
                for k, nid in ids_of.items():
                    new_index[k] = new_dense[nid]
                if targets is not None:
                    tg[t] = state["dense"][targets[t]]
                    new_index[int(forest.roots[t])] = 0xFFFFFFFF
            try:
                if self.device_forest:
                    resident.graft_forest(forest, tg, new_index)
                else:
                    resident.graft(forest.view_struct(), tg, new_index)
                state["dense"] = new_dense
                if self.encoded_store is not None:
                    for ids_of in maps:
                        self._enc_put.update(ids_of.values())
            except _lib.ArroyHipError:
                state["ok"] = False
        # the descendants the routing touched and that no longer fit (`fit_in_descendant`, :474-477, 787-795) are
        # re-split (incremental_index_large_descendant, :660-739); untouched ones are left alone, whatever their size
        large = [nid for nid in sorted(grown) if len(trees.nodes[nid][1]) > split_after]
        if large:
            forest = ds.build_subtrees([trees.nodes[nid][1] for nid in large], self._seeds(len(large)), split_after,
                                       resident=self.device_forest and state["ok"])
            maps = []
            for t, nid in enumerate(large):
                trees.import_tree(forest, t, root_id=nid)  # the sub-tree's root keeps the descendant's id (:693-702)
                maps.append(trees.last_import)
            graft(forest, maps, large)
            forest.close()
        # missing trees (:556-561)
        missing = want - len(trees.roots)
        if missing > 0 and self._group is not None:
            state["ok"] = False  # (a group build streams its trees: the index is made from the view afterwards)
        self._add_trees(ds, trees, missing, split_after, grafted=(lambda f, m: graft(f, m, None)) if state["ok"] else None,
                        resident=self.device_forest and state["ok"])
        if state["ok"]:
            live = state["dense"]
            kept = {nid: live[nid] for nid in trees.nodes}
            if self.device_compact:
                # the waste of the resident index (Index.footprint) is taken out once it outweighs what is live.  A refusal
                # (a filter of a Reader still alive) or any other failure is not a failure of the build: Index.compact is
                # all or nothing, the index stays as it was and stays correct
                try:
                    if compaction_due(resident.footprint()):
                        stats, new_of_old = resident.compact(want_map=True)
                        if stats["moved"]:
                            kept = {nid: int(new_of_old[i]) for nid, i in kept.items()}
                            st.device_compactions += 1
                except _lib.ArroyHipError:
                    pass
            return (None, None, None, None, kept)
        if resident is not None:
            resident.close()
        return None


def _assert_audit(report: dict, trees: Optional[TreeStore]) -> None:
    """Raise AssertionError for an audit report (Index.audit / audit_view) with findings, or whose per-tree stats are not
    those of the host's store."""
    from .dataset import audit_findings
    if not report["valid"]:
        raise AssertionError("the index is not valid: " + audit_findings(report))
    if trees is not None and "tree_stats" in report:
        want = [trees.stats(r) for r in trees.roots]
        got = [{k: t[k] for k in ("depth", "split_nodes", "dummy_normals", "descendants")} for t in report["tree_stats"]]
        if got != want:
            raise AssertionError(f"the tree stats of the index differ from the store's: {got} != {want}")


class Reader:
    """`Reader<D>` (src/reader.rs:128-298)."""

    def __init__(self, database: Database, index: int, st: _IndexState):
        self.database, self.index, self._st = database, index, st
        self.distance = database.distance

    @classmethod
    def open(cls, database: Database, index: int, version="v0.7") -> "Reader":  # src/reader.rs:138-200
        """`version`: of the database the tree bytes of an attached index (Database.attach_stored) come from — "v0.4" ..
        "v0.7" or (major, minor, patch).  Below v0.7 the nodes are decoded from the old layout, as `Reader::database_get` does
        through `GenericReadNodeCodecFromV0_4_0` (src/reader.rs:302-315), and the resident index is the upgraded one."""
        st = database._indexes.get(index)
        if st is None or st.metadata is None:
            raise MissingMetadata(index)
        if database.distance.name != st.metadata["distance"]:  # src/reader.rs:153-158
            raise UnmatchingDistance(st.metadata["distance"], database.distance.name)
        if st.updated:
            raise NeedBuild(index)
        if st.index is None and st.stored_trees is not None and st.dataset is not None:
            from .dataset import Index
            if not isinstance(version, str):
                major, minor = int(version[0]), int(version[1])
                version = "v0.7" if (major, minor) >= (0, 7) else f"v{major}.{max(minor, 4)}"
            node_ids, values = st.stored_trees
            st.index = Index.from_encoded(st.dataset, node_ids, values, st.metadata["roots"], layout=version)
        return cls(database, index, st)

    def dimensions(self) -> int:
        return self._st.metadata["dimensions"]

    def n_trees(self) -> int:
        return len(self._st.metadata["roots"])

    def n_items(self) -> int:
        return len(self._st.metadata["items"])

    def item_ids(self) -> List[int]:
        return list(self._st.metadata["items"])

    def is_empty(self) -> bool:
        return self.n_items() == 0

    def contains_item(self, item: ItemId) -> bool:
        return int(item) in self._st.items

    def item_vector(self, item: ItemId) -> Optional[np.ndarray]:  # src/reader.rs:266-276
        if int(item) not in self._st.items:
            return None
        return self._st.dataset.item_vector(int(item))

    def stats(self) -> dict:  # src/reader.rs:210-252
        tr = self._st.trees
        if tr is None and self._st.index is not None:  # opened from stored bytes: counted on the device
            keys = ("depth", "split_nodes", "dummy_normals", "descendants")
            return {"leaf": self.n_items(), "tree_stats": [{k: t[k] for k in keys} for t in self._st.index.audit(trees=True)["tree_stats"]]}
        return {"leaf": self.n_items(), "tree_stats": [tr.stats(r) for r in tr.roots] if tr else []}

    def assert_validity(self) -> None:  # src/reader.rs:509-589
        """Every tree reaches every item once, every list is ascending and holds only stored ids, and no tree node floats:
        counted on the device, on the resident index when there is one (Index.audit), else on a view of the store
        (audit_view).  Raises AssertionError with the non-zero classes and their first offenders."""
        st = self._st
        if st.index is not None:
            report = st.index.audit()
        elif st.dataset is not None and st.trees is not None:
            from .dataset import audit_view
            view, keep = st.trees.to_view(self.distance, self.dimensions())
            report = audit_view(st.dataset, view)
            del keep
        else:  # no items: the reference checks that no tree node is left
            assert st.trees is None or not st.trees.nodes, "tree nodes floating around in an index without items"
            return
        _assert_audit(report, None)

    def nns(self, count: int) -> "QueryBuilder":  # src/reader.rs:296-298
        return QueryBuilder(self, int(count))

    def make_filter(self, ids) -> "Filter":
        """A candidate set resident on the device for `nns(..).candidates(filter)`: made once, used by any number of queries."""
        return self._st.index.make_filter(ids)

    def make_filter_bitmap(self, words, n_bits: int) -> "Filter":
        """The same from a bitmap (uint64 words, bit i of the set = id i): a dense set need not be expanded into an id list.
        Filters of one reader combine on the device with `&`, `|`, `-` and `~`."""
        return self._st.index.make_filter_bitmap(words, n_bits)

    def make_filter_roaring(self, blob) -> "Filter":
        """The same from the bytes of a serialized RoaringBitmap (`RoaringBitmap::serialize_into`): no walk over the ids on the
        host, the containers are expanded on the device."""
        return self._st.index.make_filter_roaring(blob)

    def make_filters_roaring(self, blobs):
        """One filter per serialized RoaringBitmap in one call -> (filters, stats): Index.make_filters_roaring."""
        return self._st.index.make_filters_roaring(blobs)


class QueryBuilder:
    """`QueryBuilder` (src/reader.rs:26-124)."""

    def __init__(self, reader: Reader, count: int):
        self._r, self._count = reader, count
        self._search_k: Optional[int] = None
        self._oversampling: Optional[int] = None
        self._candidates = None  # a set of ids, or a Filter

    def search_k(self, n: int) -> "QueryBuilder":
        self._search_k = int(n)
        return self

    def oversampling(self, n: int) -> "QueryBuilder":
        self._oversampling = int(n)
        return self

    def candidates(self, ids) -> "QueryBuilder":
        """An iterable of item ids, a `Filter` of this reader's index (`Reader.make_filter`) kept across queries, or the bytes
        of a serialized RoaringBitmap (bytes / bytearray / memoryview: `Reader.make_filter_roaring` for this query, closed
        after it)."""
        self._candidates = ids if isinstance(ids, (Filter, bytes, bytearray, memoryview)) else set(int(i) for i in ids)
        return self

    def by_item(self, item: ItemId) -> Optional[List[Tuple[int, float]]]:  # src/reader.rs:46-51
        if int(item) not in self._r._st.items:
            return None
        return self._nns(item=int(item))

    def by_vector(self, vector: Sequence[float]) -> List[Tuple[int, float]]:  # src/reader.rs:64-75
        v = np.ascontiguousarray(vector, dtype=np.float32).ravel()
        if v.size != self._r.dimensions():
            raise InvalidVecDimension(self._r.dimensions(), v.size)
        return self._nns(vector=v)

    # nns_by_leaf, src/reader.rs:317-401 — the whole thing runs on device (ah_search_batch)
    def _nns(self, vector: Optional[np.ndarray] = None, item: Optional[int] = None):
        r, st = self._r, self._r._st
        if r.is_empty():
            return []
        cand, own = self._candidates, None
        if isinstance(cand, (bytes, bytearray, memoryview)):  # a serialized RoaringBitmap: a filter for this query alone
            cand = own = st.index.make_filter_roaring(cand)
        try:
            res = st.index.search(self._count, queries=None if vector is None else vector[None, :],
                                  items=None if item is None else [item],
                                  search_k=0 if self._search_k is None else self._search_k,
                                  oversampling=0 if self._oversampling is None else self._oversampling,
                                  candidates=cand)
        finally:
            if own is not None:
                own.close()
        return res[0]
