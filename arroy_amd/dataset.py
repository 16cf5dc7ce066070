"""`Dataset` / `Forest`: numpy-facing wrappers of the C ABI handles (ah_dataset / ah_forest).

`Dataset` is the HBM-resident image of what arroy calls `ImmutableLeafs` (src/parallel.rs:262-312);
every method is one C-ABI call, all arithmetic happens in HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .distances import BY_METRIC, Distance


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _blob_u8(blob) -> np.ndarray:
    """The bytes of a serialized bitmap where they lie (bytes, bytearray, memoryview, a contiguous uint8 array at any address)."""
    if isinstance(blob, np.ndarray):
        if blob.dtype != np.uint8 or not blob.flags.c_contiguous:
            raise ValueError("a serialized bitmap as an array is contiguous uint8")
        return blob.ravel()
    return np.frombuffer(blob, dtype=np.uint8)


def _update_rows(dimensions: int, up: np.ndarray, vectors) -> Optional[np.ndarray]:
    if up.size == 0:
        return None
    v = _f32(vectors)
    if v.ndim != 2 or v.shape[1] != dimensions:
        got = v.shape[1] if v.ndim == 2 else v.size
        raise _lib.InvalidVecDimension(1, f"invalid vector dimensions, provided {got} but expected {dimensions}")
    if v.shape[0] != up.size:
        raise ValueError("ids and vectors disagree on the number of items")
    return v


def _record_pointers(records: Sequence[bytes]):
    """(pointer array, record length, keep-alive) for the record calls; deliberately misaligned copies, as upload_records."""
    if not len(records):
        return None, 0, None
    rec_len = len(records[0])
    keep = [C.create_string_buffer(b"\0" + bytes(r), rec_len + 1) for r in records]
    return (C.c_void_p * len(records))(*[C.addressof(b) + 1 for b in keep]), rec_len, keep


class Dataset:
    def __init__(self, distance: type[Distance], dimensions: int, capacity: int, device: int = 0, _handle=None,
                 _finalized: bool = False, _owner=None):
        self._owner = _owner  # a DatasetGroup whose member this is (borrowed handle: the group frees it)
        self.distance = distance
        self.metric = distance.metric
        self.dimensions = int(dimensions)
        self.device = int(device)
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            _lib.check(_lib.lib().ah_dataset_create(self.metric, self.dimensions, int(capacity), device, C.byref(self._h)))
        self.finalized = _finalized

    def replicate(self, device: int) -> "Dataset":
        """A replica on another GPU of the node, copied device to device (ah_dataset_replicate): the multi-GPU build
        shards trees over replicas of the read-only dataset."""
        h = C.c_void_p()
        _lib.check(_lib.lib().ah_dataset_replicate(self._h, int(device), C.byref(h)))
        return Dataset(self.distance, self.dimensions, 0, device=device, _handle=h, _finalized=self.finalized)

    # -- staging ---------------------------------------------------------------------------------
    def upload_vectors(self, item_ids: Sequence[int], vectors) -> None:
        """`Writer::add_item` for a batch (src/writer.rs:380-394)."""
        ids = _u32(item_ids)
        v = _f32(vectors)
        if v.ndim != 2 or v.shape[1] != self.dimensions:
            got = v.shape[1] if v.ndim == 2 else v.size
            raise _lib.InvalidVecDimension(1, f"invalid vector dimensions, provided {got} but expected "
                                              f"{self.dimensions}")  # src/error.rs:17-23
        if v.shape[0] != ids.size:
            raise ValueError("ids and vectors disagree on the number of items")
        _lib.check(_lib.lib().ah_dataset_upload_vectors(self._h, _ptr(ids), _ptr(v), ids.size))

    def upload_records(self, item_ids: Sequence[int], records: Sequence[bytes], preprocessed: Optional[bool] = None) -> None:
        """Stored item records `[0u8][header][vector]` as they sit in LMDB pages (src/node.rs:224-228).
        `preprocessed` (DotProduct only): True = the headers come from a built database, i.e. `DotProduct::preprocess`
        already ran over them (ah_dataset_set_preprocessed); False = freshly added items ({0, 0} headers); None (default)
        leaves the dataset's flag alone, so a build over records nobody vouched for fails with AH_ERR_NEED_PREPROCESS
        instead of silently using extra_dim = 0."""
        ids = _u32(item_ids)
        n = ids.size
        if self.metric == 3 and preprocessed is not None:
            _lib.check(_lib.lib().ah_dataset_set_preprocessed(self._h, 1 if preprocessed else 0))
        if n == 0:
            return
        rec_len = len(records[0])
        # deliberately misaligned copies: LMDB hands out pointers at page+16+... (SURVEY.md §7 hard part 4)
        keep = [C.create_string_buffer(b"\0" + bytes(r), rec_len + 1) for r in records]
        ptrs = (C.c_void_p * n)(*[C.addressof(b) + 1 for b in keep])
        _lib.check(_lib.lib().ah_dataset_upload_records(self._h, _ptr(ids), ptrs, rec_len, n))

    # -- updates of a finalized dataset -------------------------------------------------------------
    def update_vectors(self, remove_ids: Sequence[int], upsert_ids: Sequence[int], vectors) -> None:
        """ah_dataset_update_vectors: `remove_ids` leave (absent ids are ignored), then `upsert_ids` are written with `vectors`
        (replacing their rows or adding new ones); both lists ascending.  Only these rows are staged; the dataset then behaves
        like one staged afresh with the resulting items (DotProduct: call preprocess_dot again)."""
        rm, up = _u32(remove_ids), _u32(upsert_ids)
        v = _update_rows(self.dimensions, up, vectors)
        _lib.check(_lib.lib().ah_dataset_update_vectors(self._h, _ptr(rm), rm.size, _ptr(up), _ptr(v), up.size))

    def update_records(self, remove_ids: Sequence[int], upsert_ids: Sequence[int], records: Sequence[bytes]) -> None:
        """ah_dataset_update_records: update_vectors with stored records `[0u8][header][vector]` (see upload_records)."""
        rm, up = _u32(remove_ids), _u32(upsert_ids)
        ptrs, rec_len, _keep = _record_pointers(records)
        _lib.check(_lib.lib().ah_dataset_update_records(self._h, _ptr(rm), rm.size, _ptr(up), ptrs, rec_len, up.size))

    def update_paths(self) -> dict:
        """ah_debug_update_paths: how the updates so far were applied (in place / appended / merged into new arrays)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(_lib.lib().ah_debug_update_paths(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"in_place": a.value, "appended": b.value, "merged": c.value}

    def reserve_build(self, n_trees: int, split_after: int = 0) -> None:
        """ah_dataset_reserve_build: while the records are still being staged, obtain the device memory the first build will
        ask for (fresh HBM can cost the driver tens of ms per GB) and park it in the library's device cache."""
        _lib.check(_lib.lib().ah_dataset_reserve_build(self._h, int(n_trees), int(split_after)))

    def fill_synthetic(self, seed: int, distribution: int, n_items: int) -> None:
        _lib.check(_lib.lib().ah_dataset_fill_synthetic(self._h, seed, distribution, n_items))

    def finalize(self) -> "Dataset":
        _lib.check(_lib.lib().ah_dataset_finalize(self._h))
        self.finalized = True
        return self

    def __len__(self) -> int:
        n = C.c_uint64(0)
        _lib.check(_lib.lib().ah_dataset_len(self._h, C.byref(n)))
        return int(n.value)

    def item_vector(self, item_id: int) -> np.ndarray:
        out = np.zeros(self.dimensions, dtype=np.float32)
        _lib.check(_lib.lib().ah_dataset_item_vector(self._h, item_id, _ptr(out)))
        return out

    def read_headers(self, first_row: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = len(self) - first_row if n is None else n
        hf = self.distance.header_size() // 4
        out = np.zeros((n, hf), dtype=np.float32)
        _lib.check(_lib.lib().ah_dataset_read_headers(self._h, first_row, n, _ptr(out)))
        return out

    def preprocess_dot(self) -> np.float32:
        m = C.c_float(0)
        _lib.check(_lib.lib().ah_preprocess_dot(self._h, C.byref(m)))
        return np.float32(m.value)

    # -- search side -------------------------------------------------------------------------------
    def distances(self, query=None, item: Optional[int] = None, ids=None, n: Optional[int] = None) -> np.ndarray:
        ids_a = None if ids is None else _u32(ids)
        n = (len(self) if n is None else n) if ids_a is None else ids_a.size
        out = np.zeros(n, dtype=np.float32)
        if query is not None:
            q = self._check_query(query)
            _lib.check(_lib.lib().ah_distances_by_vector(self._h, _ptr(q), _ptr(ids_a), n, _ptr(out)))
        else:
            _lib.check(_lib.lib().ah_distances_by_item(self._h, int(item), _ptr(ids_a), n, _ptr(out)))
        return out

    def rerank(self, k: int, query=None, item: Optional[int] = None, sorted_ids=None):
        ids_a = None if sorted_ids is None else _u32(sorted_ids)
        n = len(self) if ids_a is None else ids_a.size
        kk = max(1, min(int(k), n)) if n else 1
        oi = np.zeros(kk, dtype=np.uint32)
        od = np.zeros(kk, dtype=np.float32)
        on = C.c_size_t(0)
        if query is not None:
            q = self._check_query(query)
            _lib.check(_lib.lib().ah_rerank_by_vector(self._h, _ptr(q), _ptr(ids_a), n, int(k), _ptr(oi), _ptr(od),
                                                      C.byref(on)))
        else:
            _lib.check(_lib.lib().ah_rerank_by_item(self._h, int(item), _ptr(ids_a), n, int(k), _ptr(oi), _ptr(od),
                                                    C.byref(on)))
        return oi[: on.value].copy(), od[: on.value].copy()

    def rerank_batch(self, queries, id_lists, k: int):
        """`id_lists`: one ascending id list per query, or the C ABI's own shape `(ids, offsets)` (concatenated
        u32 ids + nq+1 u64 offsets) when the caller already holds it."""
        q = _f32(queries)
        if q.ndim != 2 or q.shape[1] != self.dimensions:
            raise _lib.InvalidVecDimension(1, "invalid query dimensions")
        nq = q.shape[0]
        if isinstance(id_lists, tuple):
            ids, offsets = _u32(id_lists[0]), np.ascontiguousarray(id_lists[1], dtype=np.uint64)
            assert offsets.size == nq + 1 and int(offsets[-1]) == ids.size
        else:
            offsets = np.zeros(nq + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum([len(l) for l in id_lists])
            ids = _u32(np.concatenate([_u32(l) for l in id_lists])) if nq else np.zeros(0, np.uint32)
        oi = np.zeros((nq, k), dtype=np.uint32)
        od = np.zeros((nq, k), dtype=np.float32)
        oc = np.zeros(nq, dtype=np.uint32)
        _lib.check(_lib.lib().ah_rerank_batch(self._h, _ptr(q), nq, _ptr(ids), _ptr(offsets), k, _ptr(oi), _ptr(od),
                                              _ptr(oc)))
        return oi, od, oc

    def rerank_stats(self, reset: bool = False) -> dict:
        """ah_dataset_rerank_stats: where ah_rerank_batch's wall time went (kept while the tunable AH_RERANK_TIMING is 1)."""
        st = _lib.AhRerankStats()
        _lib.check(_lib.lib().ah_dataset_rerank_stats(self._h, C.byref(st), 1 if reset else 0))
        return {f: getattr(st, f) for f, _ in _lib.AhRerankStats._fields_}

    def packed_info(self) -> dict:
        """ah_dataset_packed_info: whether the scan's packed copy of the rows exists, and how many of its rows stay f32."""
        present, raw = C.c_int(0), C.c_uint64(0)
        _lib.check(_lib.lib().ah_dataset_packed_info(self._h, C.byref(present), C.byref(raw)))
        return {"present": bool(present.value), "raw_rows": raw.value}

    def packed_rows(self) -> dict:
        """ah_dataset_packed_rows: packed_info plus the rows of the copy stored in the 24-bit fixed-point (grid) form."""
        present, raw, grid = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(_lib.lib().ah_dataset_packed_rows(self._h, C.byref(present), C.byref(raw), C.byref(grid)))
        return {"present": bool(present.value), "raw_rows": raw.value, "grid_rows": grid.value}

    def query_screen_verify(self, reset: bool = False) -> dict:
        """ah_debug_query_screen_verify: under the tunable AH_SCREEN_VERIFY=1, the candidates of the search and re-rank screens
        checked in f32, and those whose reference distance fell outside the screen's interval (must be 0)."""
        checked, bad = C.c_uint64(0), C.c_uint64(0)
        _lib.check(_lib.lib().ah_debug_query_screen_verify(self._h, C.byref(checked), C.byref(bad), 1 if reset else 0))
        return {"checked": checked.value, "violations": bad.value}

    # -- build side --------------------------------------------------------------------------------
    def split_sides(self, normal_vector: np.ndarray, normal_header, sorted_ids=None, want_margins: bool = True):
        """The margin loop (src/writer.rs:1201-1207). Returns (sides u8 per item, n_left, margins)."""
        ids_a = None if sorted_ids is None else _u32(sorted_ids)
        n = len(self) if ids_a is None else ids_a.size
        nv = np.ascontiguousarray(normal_vector).view(np.uint8)
        assert nv.size == self.distance.vector_size(self.dimensions)
        nh = np.zeros(2, dtype=np.float32)
        h = _f32(normal_header).ravel()
        nh[: h.size] = h
        bits = np.zeros((n + 7) // 8, dtype=np.uint8)
        margins = np.zeros(n, dtype=np.float32) if want_margins else None
        nl = C.c_uint64(0)
        _lib.check(_lib.lib().ah_split_sides(self._h, _ptr(nv), _ptr(nh), _ptr(ids_a), n, _ptr(bits), C.byref(nl),
                                             _ptr(margins)))
        sides = np.unpackbits(bits, bitorder="little")[:n]
        return sides, int(nl.value), margins

    def margins(self, leaf_vector: np.ndarray, leaf_header, item_ids=None) -> np.ndarray:
        """ah_margins: `D::margin(&normal, query_leaf)` (src/reader.rs:366-369) where the ITEMS of this dataset are split-plane
        normals (header = the normal's header).  The leaf is in the metric's codec: by_vector codec + `D::new_header`, by_item
        the stored item.  item_ids None: every normal in row order."""
        ids_a = None if item_ids is None else _u32(item_ids)
        n = len(self) if ids_a is None else ids_a.size
        lv = np.ascontiguousarray(leaf_vector).view(np.uint8)
        assert lv.size == self.distance.vector_size(self.dimensions)
        lh = np.zeros(2, dtype=np.float32)
        h = _f32(leaf_header).ravel()
        lh[: h.size] = h
        out = np.zeros(n, dtype=np.float32)
        _lib.check(_lib.lib().ah_margins(self._h, _ptr(lv), _ptr(lh), _ptr(ids_a), n, _ptr(out)))
        return out

    def create_split(self, sample_ids: Sequence[int]):
        """`D::create_split` with host-supplied samples (choose_two + 10 x choose)."""
        s = _u32(sample_ids)
        assert s.size == _lib.AH_SPLIT_SAMPLES
        nv = np.zeros(self.distance.vector_size(self.dimensions), dtype=np.uint8)
        nh = np.zeros(2, dtype=np.float32)
        _lib.check(_lib.lib().ah_create_split(self._h, _ptr(s), _ptr(nv), _ptr(nh)))
        return nv, nh[: self.distance.header_size() // 4].copy()

    def upload_record_pointers(self, item_ids, addresses, record_len: int) -> None:
        """ah_dataset_upload_records with raw addresses (e.g. into an mmap of an LMDB data file: the real, arbitrarily
        misaligned pointers `ImmutableLeafs::new` collects, src/parallel.rs:271-293)."""
        ids = _u32(item_ids)
        ptrs = (C.c_void_p * ids.size)(*[int(a) for a in addresses])
        _lib.check(_lib.lib().ah_dataset_upload_records(self._h, _ptr(ids), ptrs, int(record_len), ids.size))

    def build_forest(self, tree_seeds: Sequence[int], split_after: int = 0, cancel=None, progress=None,
                     max_trees_in_flight: int = 0, margin_mode: int = 0, max_host_threads: int = 0,
                     resident: bool = False) -> "Forest":
        """ah_build_forest; resident=True: ah_build_forest_resident — the same forest, which also keeps the arrays an index
        holds of it on the device (Forest.resident) for Index.from_forest / Index.graft_forest."""
        seeds = np.ascontiguousarray(tree_seeds, dtype=np.uint64)
        opt = _lib.AhBuildOptions()
        opt.n_trees = seeds.size
        opt.split_after = int(split_after)
        opt.tree_seeds = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
        cflag = C.c_int(0)
        opt.cancel = C.pointer(cflag)
        keep = None
        watcher_stop = None
        if progress is not None:
            def _cb(_user, level, nodes_done, items_routed):
                progress(level, nodes_done, items_routed)
            keep = _lib.PROGRESS_FN(_cb)
            opt.progress = keep
        if cancel is not None:
            # `cancel` is arroy's `Fn() -> bool` (src/writer.rs:100,117-123).  The library polls a flag while the level's
            # kernels run; a watcher thread evaluates the closure meanwhile (ctypes releases the GIL during the call).
            import threading
            if cancel():  # polled before the first level too (src/writer.rs:1178)
                cflag.value = 1
            watcher_stop = threading.Event()

            def _watch():
                while not watcher_stop.wait(0.0005):
                    if cancel():
                        cflag.value = 1
                        return
            threading.Thread(target=_watch, daemon=True).start()
        opt.max_trees_in_flight = int(max_trees_in_flight)
        opt.margin_mode = int(margin_mode)
        opt.max_host_threads = int(max_host_threads)
        h = C.c_void_p()
        try:
            build = _lib.lib().ah_build_forest_resident if resident else _lib.lib().ah_build_forest
            _lib.check(build(self._h, C.byref(opt), C.byref(h)))
        finally:
            if watcher_stop is not None:
                watcher_stop.set()
        return Forest(h, self.distance, self.dimensions)

    def build_forest_stream(self, tree_seeds: Sequence[int], sink=None, split_after: int = 0, margin_mode: int = 0,
                            max_trees_in_flight: int = 0, max_host_threads: int = 0, encoded: bool = False, node_id_base: int = 0):
        """ah_build_forest_stream: the node sink DURING the build (`TmpNodes::put`, src/parallel.rs:130-147).  `sink(batch)`
        receives every `_lib.AhNodeBatch` (valid only during the call; return non-zero to stop the build); with sink=None the
        batches are collected into a `StreamedForest`.  Returns (roots, stats, collected or None).
        encoded=True: ah_build_forest_stream_encoded — the payloads are NodeCodec values encoded on the device and every node
        id has `node_id_base` added (`roots` too; a StreamedForest keeps ids minus the base)."""
        if node_id_base and not encoded:
            raise ValueError("node_id_base belongs to the encoded stream")
        seeds = np.ascontiguousarray(tree_seeds, dtype=np.uint64)
        opt = _lib.AhBuildOptions()
        opt.n_trees = seeds.size
        opt.split_after = int(split_after)
        opt.tree_seeds = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
        opt.margin_mode = int(margin_mode)
        opt.max_trees_in_flight = int(max_trees_in_flight)
        opt.max_host_threads = int(max_host_threads)
        collected = StreamedForest(self.distance, self.dimensions, node_id_base=int(node_id_base)) if sink is None else None
        fn = collected.take if sink is None else sink
        failure = []

        def _cb(_user, batch_p):
            try:
                return int(fn(batch_p.contents) or 0)
            except BaseException as e:  # noqa: BLE001 — nothing may unwind through the C frames
                failure.append(e)
                return -1
        cb = _lib.NODE_BATCH_FN(_cb)
        roots = np.zeros(seeds.size, dtype=np.uint32)
        st = _lib.AhBuildStats()
        if encoded:
            enc = _lib.AhEncodeOptions(int(node_id_base), 0)
            code = _lib.lib().ah_build_forest_stream_encoded(self._h, C.byref(opt), C.byref(enc), cb, None, _ptr(roots), C.byref(st))
        else:
            code = _lib.lib().ah_build_forest_stream(self._h, C.byref(opt), cb, None, _ptr(roots), C.byref(st))
        if failure:
            raise failure[0]
        _lib.check(code)
        stats = {f: getattr(st, f) for f, _ in _lib.AhBuildStats._fields_}
        stats["margin_mode_launches"] = list(st.margin_mode_launches)
        if collected is not None:
            collected.roots = roots - np.uint32(node_id_base)
        return roots, stats, collected

    def encode_descendants(self, id_lists: Sequence[Sequence[int]], sizes_only: bool = False, out_cap: int | None = None):
        """ah_encode_descendants: the Descendants values (tag byte included) of ascending id lists, encoded on the device.
        Returns a list of bytes, or with sizes_only the value offsets (len(id_lists) + 1, uint64)."""
        n = len(id_lists)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(l) for l in id_lists])
        ids = _u32(np.concatenate([_u32(l) for l in id_lists])) if n else np.zeros(0, np.uint32)
        if ids.size == 0:
            ids = np.zeros(1, np.uint32)
        ends = np.zeros(n + 1, dtype=np.uint64)
        _lib.check(_lib.lib().ah_encode_descendants(self._h, _ptr(ids), _ptr(offsets), n, None, 0, _ptr(ends)))
        if sizes_only:
            return ends
        cap = int(ends[n]) if out_cap is None else int(out_cap)
        out = np.full(int(ends[n]) + 64, 0xA5, dtype=np.uint8)  # (the tail shows a write past the cap)
        _lib.check(_lib.lib().ah_encode_descendants(self._h, _ptr(ids), _ptr(offsets), n, _ptr(out), cap, _ptr(ends)))
        assert bool(np.all(out[int(ends[n]):] == 0xA5)), "ah_encode_descendants wrote past the end of its values"
        return [out[int(ends[i]): int(ends[i + 1])].tobytes() for i in range(n)]

    def build_subtrees(self, id_lists: Sequence[Sequence[int]], tree_seeds: Sequence[int], split_after: int = 0,
                       resident: bool = False) -> "Forest":
        """`incremental_index_large_descendant` for many item subsets at once (ah_build_subtrees; resident=True:
        ah_build_subtrees_resident, see build_forest)."""
        seeds = np.ascontiguousarray(tree_seeds, dtype=np.uint64)
        assert seeds.size == len(id_lists)
        offsets = np.zeros(len(id_lists) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(l) for l in id_lists])
        ids = _u32(np.concatenate([_u32(l) for l in id_lists])) if len(id_lists) else np.zeros(1, np.uint32)
        opt = _lib.AhBuildOptions()
        opt.n_trees = seeds.size
        opt.split_after = int(split_after)
        opt.tree_seeds = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
        h = C.c_void_p()
        build = _lib.lib().ah_build_subtrees_resident if resident else _lib.lib().ah_build_subtrees
        _lib.check(build(self._h, C.byref(opt), _ptr(ids), _ptr(offsets), C.byref(h)))
        return Forest(h, self.distance, self.dimensions)

    def create_index(self, forest: "Forest") -> "Index":
        """Mirror `forest` in HBM next to this dataset (ah_index_create)."""
        return Index(self, forest)

    # -- measurement -------------------------------------------------------------------------------
    def bench_scan(self, query_item: int, n: int, iterations: int, want_out: bool = False):
        out = np.zeros(n, dtype=np.float32) if want_out else None
        ms = C.c_double(0)
        _lib.check(_lib.lib().ah_bench_scan(self._h, query_item, n, iterations, _ptr(out), C.byref(ms)))
        return ms.value, out

    # -- plumbing ----------------------------------------------------------------------------------
    def _check_query(self, query) -> np.ndarray:
        q = _f32(query).ravel()
        if q.size != self.dimensions:  # src/reader.rs:64-69
            raise _lib.InvalidVecDimension(1, f"invalid vector dimensions, provided {q.size} but expected "
                                              f"{self.dimensions}")
        return q

    def close(self) -> None:
        if self._h:
            if self._owner is None:
                _lib.lib().ah_dataset_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DatasetGroup:
    """One replica of a dataset per listed device (ah_group): staged from one host pass, one forest built on all of them —
    tree t on member t mod G, the forest a single Dataset builds with the same seeds.  `devices` may repeat a device."""

    def __init__(self, distance: type[Distance], dimensions: int, capacity: int, devices: Sequence[int]):
        self.distance = distance
        self.metric = distance.metric
        self.dimensions = int(dimensions)
        self.devices = [int(d) for d in devices]
        self._h = C.c_void_p()
        arr = (C.c_int * max(1, len(self.devices)))(*self.devices)
        _lib.check(_lib.lib().ah_group_create(self.metric, self.dimensions, int(capacity), arr, len(self.devices),
                                              C.byref(self._h)))
        self.finalized = False
        self._members = {}

    def __len__(self) -> int:
        return len(self.devices)

    def upload_vectors(self, item_ids: Sequence[int], vectors) -> None:
        """Dataset.upload_vectors for every member: each chunk is gathered once and sent to every device."""
        ids = _u32(item_ids)
        v = _f32(vectors)
        if v.ndim != 2 or v.shape[1] != self.dimensions:
            got = v.shape[1] if v.ndim == 2 else v.size
            raise _lib.InvalidVecDimension(1, f"invalid vector dimensions, provided {got} but expected {self.dimensions}")
        if v.shape[0] != ids.size:
            raise ValueError("ids and vectors disagree on the number of items")
        _lib.check(_lib.lib().ah_group_upload_vectors(self._h, _ptr(ids), _ptr(v), ids.size))

    def upload_records(self, item_ids: Sequence[int], records: Sequence[bytes], preprocessed: Optional[bool] = None) -> None:
        """Dataset.upload_records for every member."""
        ids = _u32(item_ids)
        n = ids.size
        if self.metric == 3 and preprocessed is not None:
            _lib.check(_lib.lib().ah_group_set_preprocessed(self._h, 1 if preprocessed else 0))
        if n == 0:
            return
        rec_len = len(records[0])
        keep = [C.create_string_buffer(b"\0" + bytes(r), rec_len + 1) for r in records]
        ptrs = (C.c_void_p * n)(*[C.addressof(b) + 1 for b in keep])
        _lib.check(_lib.lib().ah_group_upload_records(self._h, _ptr(ids), ptrs, rec_len, n))

    def flush(self) -> None:
        _lib.check(_lib.lib().ah_group_upload_flush(self._h))

    def update_vectors(self, remove_ids: Sequence[int], upsert_ids: Sequence[int], vectors) -> None:
        """Dataset.update_vectors for every member: the upserted rows are gathered once and sent to every device."""
        rm, up = _u32(remove_ids), _u32(upsert_ids)
        v = _update_rows(self.dimensions, up, vectors)
        _lib.check(_lib.lib().ah_group_update_vectors(self._h, _ptr(rm), rm.size, _ptr(up), _ptr(v), up.size))

    def update_records(self, remove_ids: Sequence[int], upsert_ids: Sequence[int], records: Sequence[bytes]) -> None:
        """Dataset.update_records for every member."""
        rm, up = _u32(remove_ids), _u32(upsert_ids)
        ptrs, rec_len, _keep = _record_pointers(records)
        _lib.check(_lib.lib().ah_group_update_records(self._h, _ptr(rm), rm.size, _ptr(up), ptrs, rec_len, up.size))

    def reserve_build(self, n_trees: int, split_after: int = 0) -> None:
        _lib.check(_lib.lib().ah_group_reserve_build(self._h, int(n_trees), int(split_after)))

    def preprocess_dot(self) -> np.float32:
        m = C.c_float(0)
        _lib.check(_lib.lib().ah_group_preprocess_dot(self._h, C.byref(m)))
        return np.float32(m.value)

    def finalize(self) -> "DatasetGroup":
        _lib.check(_lib.lib().ah_group_finalize(self._h))
        self.finalized = True
        for m in self._members.values():
            m.finalized = True
        return self

    def member(self, i: int) -> Dataset:
        """Member i as a Dataset (borrowed: it lives as long as the group; reading calls only)."""
        if i not in self._members:
            h = C.c_void_p()
            _lib.check(_lib.lib().ah_group_member(self._h, int(i), C.byref(h)))
            self._members[i] = Dataset(self.distance, self.dimensions, 0, device=self.devices[i], _handle=h,
                                       _finalized=self.finalized, _owner=self)
        return self._members[i]

    def build_stream(self, tree_seeds: Sequence[int], sink=None, split_after: int = 0, margin_mode: int = 0,
                     max_trees_in_flight: int = 0, max_host_threads: int = 0, cancel=None, progress=None):
        """ah_build_forest_group_stream: the whole forest over the members, streamed to `sink(batch)` with the contract of
        Dataset.build_forest_stream (sink=None collects a StreamedForest).  `cancel`: a ctypes c_int the caller may raise;
        `progress(level, nodes_done, items_routed)`.  Returns (roots, summed stats, per-member stats, collected or None)."""
        seeds = np.ascontiguousarray(tree_seeds, dtype=np.uint64)
        opt = _lib.AhBuildOptions()
        opt.n_trees = seeds.size
        opt.split_after = int(split_after)
        opt.tree_seeds = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
        opt.margin_mode = int(margin_mode)
        opt.max_trees_in_flight = int(max_trees_in_flight)
        opt.max_host_threads = int(max_host_threads)
        if cancel is not None:
            opt.cancel = C.pointer(cancel)
        keep = None
        if progress is not None:
            def _pcb(_user, level, nodes_done, items_routed):
                try:
                    progress(level, nodes_done, items_routed)
                except BaseException:  # noqa: BLE001 — nothing may unwind through the C frames
                    pass
            keep = _lib.PROGRESS_FN(_pcb)
            opt.progress = keep
        collected = StreamedForest(self.distance, self.dimensions) if sink is None else None
        fn = collected.take if sink is None else sink
        failure = []

        def _cb(_user, batch_p):
            try:
                return int(fn(batch_p.contents) or 0)
            except BaseException as e:  # noqa: BLE001
                failure.append(e)
                return -1
        cb = _lib.NODE_BATCH_FN(_cb)
        roots = np.zeros(seeds.size, dtype=np.uint32)
        st = _lib.AhBuildStats()
        per = (_lib.AhBuildStats * len(self.devices))()
        code = _lib.lib().ah_build_forest_group_stream(self._h, C.byref(opt), cb, None, _ptr(roots), C.byref(st), per)
        del keep
        if failure:
            raise failure[0]
        _lib.check(code)

        def _d(s):
            d = {f: getattr(s, f) for f, _ in _lib.AhBuildStats._fields_}
            d["margin_mode_launches"] = list(s.margin_mode_launches)
            return d
        if collected is not None:
            collected.roots = roots
        return roots, _d(st), [_d(s) for s in per], collected

    def close(self) -> None:
        if self._h:
            for m in self._members.values():
                m._h = C.c_void_p()
            self._members = {}
            _lib.lib().ah_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the ah_node record (include/arroy_hip.h) as a numpy dtype
_NODE_DT = np.dtype([("kind", "u1"), ("has_normal", "u1"), ("reserved", "<u2"), ("tree", "<u4"), ("left", "<u4"), ("right", "<u4"),
                     ("offset", "<u8"), ("count", "<u4"), ("depth", "<u4")], align=True)
assert _NODE_DT.itemsize == C.sizeof(_lib.AhNode)


class Index:
    """Dataset + forest resident in HBM: the whole `Reader::nns_by_leaf` runs on device (ah_search_batch)."""

    def __init__(self, dataset: Dataset, forest: Optional["Forest"], view=None):
        self.dataset = dataset
        self._h = C.c_void_p()
        self._filters = weakref.WeakSet()  # the live Filter objects of this index: closed before it
        if view is not None:  # caller-owned arrays in the ah_forest_view shape (ah_index_create_from_view)
            _lib.check(_lib.lib().ah_index_create_from_view(dataset._h, C.cast(C.byref(view), C.POINTER(_lib.AhForestView)),
                                                            C.byref(self._h)))
        else:
            _lib.check(_lib.lib().ah_index_create(dataset._h, forest._h, C.byref(self._h)))

    @classmethod
    def from_forest(cls, dataset: Dataset, forest: "Forest", new_index=None) -> "Index":
        """ah_index_create_from_forest: the index of `forest`, made from the forest's device copy where it has one (a resident
        forest on this dataset's device; the copy is consumed) and from its host view otherwise — the same index either way.
        new_index[k]: the final index of view node k (a permutation of the forest's nodes: the numbering of the host's store);
        None: the forest's own numbering, the index of Index(dataset, forest).  `from_device` on the result tells which path ran."""
        ni = None if new_index is None else _u32(new_index).ravel()
        if ni is not None and ni.size != len(forest.nodes):
            raise ValueError(f"new_index has {ni.size} entries for the {len(forest.nodes)} nodes of the forest")
        self = cls.__new__(cls)
        self.dataset = dataset
        self._h = C.c_void_p()
        self._filters = weakref.WeakSet()
        from_device = C.c_int(0)
        _lib.check(_lib.lib().ah_index_create_from_forest(dataset._h, forest._h, _ptr(ni), C.byref(from_device), C.byref(self._h)))
        self.from_device = bool(from_device.value)
        return self

    def graft_forest(self, forest: "Forest", targets, new_index=None, want_map: bool = False):
        """ah_index_graft_forest: graft() with the view of `forest`, read from the forest's device copy where it has one (consumed)
        and from its host view otherwise.  Returns from_device, with want_map (from_device, the new index of every old slot)."""
        tg = _u32(targets).ravel()
        if tg.size != forest.n_trees:
            raise ValueError(f"{tg.size} targets for the {forest.n_trees} trees of the forest")
        ni = None if new_index is None else _u32(new_index).ravel()
        if ni is not None and ni.size != len(forest.nodes):
            raise ValueError(f"new_index has {ni.size} entries for the {len(forest.nodes)} nodes of the forest")
        out = np.zeros(self.export_info()["n_nodes"], dtype=np.uint32) if want_map else None
        from_device = C.c_int(0)
        _lib.check(_lib.lib().ah_index_graft_forest(self._h, forest._h, _ptr(tg), _ptr(ni), _ptr(out), C.byref(from_device)))
        return (bool(from_device.value), out) if want_map else bool(from_device.value)

    @classmethod
    def from_encoded(cls, dataset: Dataset, node_ids, values, roots, want_stats: bool = False, layout="v0.7"):
        """ah_index_create_from_encoded: a resident index from the `NodeCodec` values LMDB stores for the tree nodes, as a
        cursor over the tree keys yields them — `node_ids` strictly ascending, `values[i]` the bytes of node_ids[i] (bytes or
        a uint8 array, at any address), `roots` the root node ids.  The values are decoded on the device; node i of the index
        is the value of the i-th id.  Returns the index, with want_stats (index, ah_index_decode_stats as a dict).
        layout "v0.5" | "v0.6" (the same layout) | "v0.4": ah_index_create_from_legacy — the values of an older database, the
        index the upgraded one (node_codec.upgrade_values: every Item child a new one-id Descendants node behind the nodes of
        the values); want_stats then gives (index, decode stats, ah_index_legacy_stats as a dict)."""
        from . import node_codec
        layout = node_codec.layout_of(layout)
        ids = _u32(node_ids)
        arrs = [_blob_u8(v) for v in values]
        if len(arrs) != ids.size:
            raise ValueError(f"{len(arrs)} values for {ids.size} node ids")
        rt = _u32(roots)
        n = len(arrs)
        ptrs = (C.c_void_p * max(1, n))(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * max(1, n))(*[a.size for a in arrs])
        self = cls.__new__(cls)
        self.dataset = dataset
        self._h = C.c_void_p()
        self._filters = weakref.WeakSet()
        st = _lib.AhIndexDecodeStats()
        args = (_ptr(ids) if n else None, ptrs, lens, n, _ptr(rt) if rt.size else None, int(rt.size), C.byref(self._h), C.byref(st))
        legacy = _lib.AhIndexLegacyStats()
        if layout == node_codec.LAYOUT_V0_7:
            _lib.check(_lib.lib().ah_index_create_from_encoded(dataset._h, *args))
        else:
            _lib.check(_lib.lib().ah_index_create_from_legacy(dataset._h, layout, *args, C.byref(legacy)))
        if not want_stats:
            return self
        stats = {k: (float if k.startswith("seconds") else int)(getattr(st, k)) for k, _ in _lib.AhIndexDecodeStats._fields_}
        if layout == node_codec.LAYOUT_V0_7:
            return self, stats
        return self, stats, {k: int(getattr(legacy, k)) for k, _ in _lib.AhIndexLegacyStats._fields_}

    def make_filter(self, ids, sorted: bool = False) -> "Filter":
        """ah_filter_create: `QueryBuilder::candidates` as an object resident on the device, for any number of searches.
        sorted=True: `ids` is already an ascending array of distinct ids (what a RoaringBitmap iterates)."""
        return Filter(self, ids, sorted)

    def make_filter_bitmap(self, words, n_bits: int) -> "Filter":
        """ah_filter_create_bitmap: a resident filter from a bitmap as the host holds it — bit i (bit i & 63 of the uint64
        words[i >> 6]) set = id i is a candidate.  Equal to make_filter of the set bits among the first `n_bits`."""
        w = np.ascontiguousarray(words, dtype=np.uint64).ravel()
        if int(n_bits) < 0 or int(n_bits) > w.size * 64:
            raise ValueError(f"n_bits = {n_bits} for {w.size} words")
        h = C.c_void_p()
        _lib.check(_lib.lib().ah_filter_create_bitmap(self._h, _ptr(w) if w.size else None, int(n_bits), C.byref(h)))
        return Filter._adopt(self, h)

    def make_filter_roaring(self, blob) -> "Filter":
        """ah_filter_create_roaring: a resident filter from the bytes of one serialized RoaringBitmap (`serialize_into`; the
        format: arroy_amd/roaring.py), expanded on the device.  Equal to make_filter of the ids the bitmap holds."""
        a = _blob_u8(blob)
        h = C.c_void_p()
        _lib.check(_lib.lib().ah_filter_create_roaring(self._h, a.ctypes.data, a.size, C.byref(h)))
        return Filter._adopt(self, h)

    def make_filters_roaring(self, blobs):
        """ah_filter_create_roaring_batch: one resident filter per serialized RoaringBitmap in ONE call — one upload, one
        expansion launch, the per-node counts of up to FILTER_RESUME_GROUP filters in one pass over the ids of the forest.  All
        or nothing.  -> (the filters, ah_filter_roaring_stats as a dict)."""
        arrs = [_blob_u8(b) for b in blobs]
        n = len(arrs)
        ptrs = (C.c_void_p * max(1, n))(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * max(1, n))(*[a.size for a in arrs])
        handles = (C.c_void_p * max(1, n))()
        st = _lib.AhFilterRoaringStats()
        _lib.check(_lib.lib().ah_filter_create_roaring_batch(self._h, ptrs, lens, n, handles, C.byref(st)))
        filters = [Filter._adopt(self, C.c_void_p(handles[i])) for i in range(n)]
        return filters, {k: int(getattr(st, k)) for k, _ in _lib.AhFilterRoaringStats._fields_}

    def combine_filters(self, op, filters, want_stats: bool = False):
        """ah_filter_combine: "and" / "or" / "andnot" (filters[0] minus the others) / "not" (one filter) of resident filters of
        this index as a new resident filter, computed on the device; bit for bit the filter make_filter gives for the id list of
        the result.  want_stats: (filter, ah_filter_combine_stats as a dict)."""
        code = _lib.FILTER_OPS[op.lower()] if isinstance(op, str) else int(op)
        filters = list(filters)
        handles = (C.c_void_p * max(1, len(filters)))(*[f._handle() for f in filters])
        h, st = C.c_void_p(), _lib.AhFilterCombineStats()
        _lib.check(_lib.lib().ah_filter_combine(code, handles, len(filters), C.byref(h), C.byref(st)))
        f = Filter._adopt(self, h)
        return (f, {k: int(getattr(st, k)) for k, _ in _lib.AhFilterCombineStats._fields_}) if want_stats else f

    def resume_filters(self, filters, edits=None, want_stats: bool = False, edits_sorted: bool = False):
        """ah_filter_resume_batch: suspended filters of this index (Filter.suspend) back on the index as it is now, after any
        number of maintenance calls and dataset updates.  `edits`: per filter None or (remove_ids, add_ids), either of them None
        or any iterable of ids — what the host's update did to that filter's set.  Filter i becomes the filter make_filter gives
        now for ((old set - remove) | add) cut at the largest stored id; the per-node counts of up to FILTER_RESUME_GROUP filters
        are made in one pass over the ids of the forest.  All or nothing.  edits_sorted: every list is already an ascending
        array of distinct ids.  want_stats: ah_filter_resume_stats as a dict."""
        filters = list(filters)
        n = len(filters)
        if edits is not None and len(edits) != n:
            raise ValueError(f"{len(edits)} edits for {n} filters")
        for f in filters:
            if f.index is not self:
                raise ValueError("a filter of another index")
        handles = (C.c_void_p * max(1, n))(*[f._handle() for f in filters])
        keep, arr = [], None
        if edits is not None:
            arr = (_lib.AhFilterEdit * max(1, n))()
            for i, e in enumerate(edits):
                for k, ids in enumerate(e if e is not None else ()):
                    if ids is None:
                        continue
                    a = _u32(ids).ravel() if edits_sorted else _u32(sorted(set(int(c) for c in ids)))
                    keep.append(a)
                    if a.size:
                        setattr(arr[i], ("remove_sorted", "add_sorted")[k], a.ctypes.data)
                        setattr(arr[i], ("n_remove", "n_add")[k], a.size)
        st = _lib.AhFilterResumeStats()
        _lib.check(_lib.lib().ah_filter_resume_batch(handles, arr, n, C.byref(st)))
        for f in filters:
            f._suspended = False
        if want_stats:
            return {k: int(getattr(st, k)) for k, _ in _lib.AhFilterResumeStats._fields_}

    def filters_suspended(self) -> int:
        """ah_index_filters_suspended: the suspended filters of this index (a level, like filter_stats()["filters_alive"])."""
        out = C.c_uint64()
        _lib.check(_lib.lib().ah_index_filters_suspended(self._h, C.byref(out)))
        return int(out.value)

    def search(self, count: int, queries=None, items=None, search_k: int = 0, oversampling: int = 0, candidates=None,
               raw: bool = False, candidates_sorted: bool = False, filters=None, filter_of_query=None):
        """Batch of `QueryBuilder::by_vector` (queries: nq x dims) or `by_item` (items: nq ids).
        Returns a list (one entry per query) of [(id, distance), ...]; with raw=True the (ids, distances, counts)
        arrays of the C ABI (no per-result Python objects).  `candidates` = `QueryBuilder::candidates` as an id list for the
        whole call, or a `Filter`; `filters` (a list of `Filter`) with `filter_of_query` (per query an index into it, or
        NO_FILTER / -1) gives every query its own (ah_search_batch_filters)."""
        ds = self.dataset
        if queries is not None:
            q = _f32(queries)
            if q.ndim == 1:
                q = q[None, :]
            if q.shape[1] != ds.dimensions:
                raise _lib.InvalidVecDimension(1, f"Invalid vector dimensions. Got {q.shape[1]} but expected "
                                                  f"{ds.dimensions}")
            nq, it = q.shape[0], None
        else:
            it = _u32(items).ravel()
            nq, q = it.size, None
        if isinstance(candidates, Filter):
            if filters is not None:
                raise ValueError("candidates= as a Filter and filters= exclude each other")
            filters, filter_of_query, candidates = [candidates], None, None
        oi = np.zeros((nq, count), dtype=np.uint32)
        od = np.zeros((nq, count), dtype=np.float32)
        oc = np.zeros(nq, dtype=np.uint32)
        if filters is not None or filter_of_query is not None:
            if candidates is not None:
                raise ValueError("candidates= as an id list and filters= exclude each other")
            filters = list(filters or [])
            handles = (C.c_void_p * max(1, len(filters)))(*[f._handle() for f in filters])
            foq = None
            if filter_of_query is not None:
                foq = np.ascontiguousarray(np.asarray(filter_of_query, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32).ravel()
                if foq.size != nq:
                    raise ValueError(f"filter_of_query has {foq.size} entries for {nq} queries")
            _lib.check(_lib.lib().ah_search_batch_filters(self._h, _ptr(q), _ptr(it), nq, int(count), int(min(search_k, 2**62)),
                                                          int(oversampling), handles, len(filters), _ptr(foq), _ptr(oi),
                                                          _ptr(od), _ptr(oc)))
        else:
            if candidates is None:
                filt = None
            elif candidates_sorted:  # already an ascending array of distinct ids (what a RoaringBitmap iterates)
                filt = _u32(candidates)
            else:
                filt = _u32(sorted(set(int(c) for c in candidates)))
            _lib.check(_lib.lib().ah_search_batch(self._h, _ptr(q), _ptr(it), nq, int(count), int(min(search_k, 2**62)),
                                                  int(oversampling), _ptr(filt), 0 if filt is None else filt.size,
                                                  0 if filt is None else 1, _ptr(oi), _ptr(od), _ptr(oc)))
        if raw:
            return oi, od, oc
        return [[(int(oi[i, j]), float(od[i, j])) for j in range(int(oc[i]))] for i in range(nq)]

    def search_params(self, counts, queries=None, items=None, search_ks=None, oversamplings=None, filters=None,
                      filter_of_query=None, raw: bool = False):
        """`search` in which every query has its own count, search_k and oversampling (ah_search_batch_params): each of the
        three is a scalar for all queries or an array of one value per query (search_ks / oversamplings None or 0: the
        reference's defaults).  Query q gets what `search` gives it alone with its values.  `filters` / `filter_of_query` as in
        `search`.  Returns a list (one entry per query) of [(id, distance), ...]; with raw=True the (ids, distances, counts)
        arrays of the C ABI, nq x max(counts), short rows padded with 0xFFFFFFFF / NaN."""
        ds = self.dataset
        if queries is not None:
            q = _f32(queries)
            if q.ndim == 1:
                q = q[None, :]
            if q.shape[1] != ds.dimensions:
                raise _lib.InvalidVecDimension(1, f"Invalid vector dimensions. Got {q.shape[1]} but expected "
                                                  f"{ds.dimensions}")
            nq, it = q.shape[0], None
        else:
            it = _u32(items).ravel()
            nq, q = it.size, None

        def per_query(values, name, limit):
            a = np.asarray(0 if values is None else values)
            if a.dtype.kind not in "iu":
                raise TypeError(f"{name} must be integers")
            a = np.full(nq, a[()]) if a.ndim == 0 else a.ravel()
            if a.size != nq:
                raise ValueError(f"{name} has {a.size} entries for {nq} queries")
            if nq and ((a.dtype.kind == "i" and (a < 0).any()) or (limit is not None and (a > limit).any())):
                raise ValueError(f"{name} must lie in 0 .. {limit if limit is not None else 2**64 - 1}")
            return a

        params = np.zeros(nq, dtype=np.dtype([("search_k", "<u8"), ("count", "<u4"), ("oversampling", "<u4")]))
        params["count"] = per_query(counts, "counts", 0xFFFFFFFF)
        params["search_k"] = per_query(search_ks, "search_ks", None)
        params["oversampling"] = per_query(oversamplings, "oversamplings", 0xFFFFFFFF)
        stride = int(params["count"].max()) if nq else 0
        oi = np.zeros((nq, stride), dtype=np.uint32)
        od = np.zeros((nq, stride), dtype=np.float32)
        oc = np.zeros(nq, dtype=np.uint32)
        filters = list(filters or [])
        handles = (C.c_void_p * max(1, len(filters)))(*[f._handle() for f in filters])
        foq = None
        if filter_of_query is not None:
            foq = np.ascontiguousarray(np.asarray(filter_of_query, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32).ravel()
            if foq.size != nq:
                raise ValueError(f"filter_of_query has {foq.size} entries for {nq} queries")
        _lib.check(_lib.lib().ah_search_batch_params(self._h, _ptr(q), _ptr(it), nq,
                                                     C.cast(params.ctypes.data, C.POINTER(_lib.AhQueryParams)), stride, handles,
                                                     len(filters), _ptr(foq), _ptr(oi), _ptr(od), _ptr(oc)))
        if raw:
            return oi, od, oc
        return [[(int(oi[i, j]), float(od[i, j])) for j in range(int(oc[i]))] for i in range(nq)]

    def params_stats(self, reset: bool = False) -> dict:
        """ah_index_params_stats: how ah_search_batch_params cut its calls."""
        st = _lib.AhParamsStats()
        _lib.check(_lib.lib().ah_index_params_stats(self._h, C.byref(st), 1 if reset else 0))
        return {f: int(getattr(st, f)) for f, _ in _lib.AhParamsStats._fields_}

    def exhausted_stats(self, reset: bool = False) -> dict:
        """ah_index_exhausted_stats: the queries AH_SEARCH_EXHAUSTED=1 answered from their filter's kept list, and the lists made."""
        st = _lib.AhExhaustedStats()
        _lib.check(_lib.lib().ah_index_exhausted_stats(self._h, C.byref(st), 1 if reset else 0))
        return {f: int(getattr(st, f)) for f, _ in _lib.AhExhaustedStats._fields_}

    def filter_stats(self, reset: bool = False) -> dict:
        """ah_index_filter_stats: how ah_search_batch_filters cut its calls, and the filters of this index."""
        st = _lib.AhFilterStats()
        _lib.check(_lib.lib().ah_index_filter_stats(self._h, C.byref(st), 1 if reset else 0))
        return {f: int(getattr(st, f)) for f, _ in _lib.AhFilterStats._fields_}

    def stats(self, reset: bool = False) -> dict:
        """ah_index_search_stats: which descent tier / dedup path / re-rank path served the searches so far."""
        st = _lib.AhSearchStats()
        _lib.check(_lib.lib().ah_index_search_stats(self._h, C.byref(st), 1 if reset else 0))
        return {f: int(getattr(st, f)) for f, _ in _lib.AhSearchStats._fields_ if f != "reserved"}

    def route_items(self, item_ids: Sequence[int], tree_seeds: Sequence[int]) -> np.ndarray:
        """Incremental routing (src/writer.rs:1398-1459): [n_trees, n] forest-local Descendants node per item."""
        ids = _u32(item_ids)
        seeds = np.ascontiguousarray(tree_seeds, dtype=np.uint64)
        out = np.zeros((seeds.size, ids.size), dtype=np.uint32)
        _lib.check(_lib.lib().ah_route_items(self._h, _ptr(ids), ids.size, _ptr(seeds), _ptr(out)))
        return out

    def delete_items(self, sorted_ids, split_after: int) -> dict:
        """ah_index_delete_items: `delete_items_from_trees` (src/writer.rs:978-1114) on the resident index.  `sorted_ids`
        ascending and distinct.  Returns the delta for the host's store (TreeStore.apply_delta), in index-local node indices:
        removed, put_index, put (kind / has_normal / left / right, or offset / count into desc), desc, roots."""
        arr = _u32(sorted_ids).ravel()
        h = C.c_void_p()
        _lib.check(_lib.lib().ah_index_delete_items(self._h, _ptr(arr), arr.size, int(split_after), C.byref(h)))
        return self._take_delta(h)

    def drop_trees(self, n_drop: int, sort_roots: bool = False) -> dict:
        """ah_index_drop_trees: `delete_extra_trees` (src/writer.rs:631-655) on the resident index, `n_drop` times
        `roots.swap_remove(0)` + `delete_tree`.  Returns a delta in the shape of delete_items (TreeStore.apply_delta applies
        it unchanged): `removed` is every node of the dropped trees, `put` is empty, `roots` the surviving roots in the order
        the swap_removes leave them, or ascending with sort_roots (for a build that calls no delete_items afterwards)."""
        if n_drop < 0:
            raise ValueError(f"n_drop = {n_drop}")
        h = C.c_void_p()
        _lib.check(_lib.lib().ah_index_drop_trees(self._h, int(n_drop), _lib.DROP_SORT_ROOTS if sort_roots else 0, C.byref(h)))
        return self._take_delta(h)

    @staticmethod
    def _take_delta(h) -> dict:
        """ah_index_delta_get as numpy arrays; the delta is destroyed."""
        try:
            v = _lib.AhIndexDeltaView()
            _lib.check(_lib.lib().ah_index_delta_get(h, C.byref(v)))

            def u32s(p, n):
                return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            n_put = int(v.n_put)
            put = np.frombuffer(C.string_at(v.put, n_put * _NODE_DT.itemsize), dtype=_NODE_DT).copy() if n_put else np.zeros(0, _NODE_DT)
            return {"removed": u32s(v.removed, int(v.n_removed)), "put_index": u32s(v.put_index, n_put), "put": put,
                    "desc": u32s(v.desc, int(v.desc_len)), "roots": u32s(v.roots, int(v.n_trees))}
        finally:
            _lib.lib().ah_index_delta_destroy(h)

    def insert_items(self, sorted_ids, tree_seeds: Sequence[int]) -> dict:
        """ah_index_insert_items: `insert_items_in_descendants_from_frozen_reader` (src/writer.rs:1398-1459) on the resident
        index, the lists included: every id (ascending, distinct, a row of the dataset) is routed as route_items routes it and
        joins the Descendants node it lands in.  Returns a delta in the shape of delete_items: `removed` is empty, `put` are
        the nodes an id landed in with their new lists."""
        arr = _u32(sorted_ids).ravel()
        seeds = np.ascontiguousarray(tree_seeds, dtype=np.uint64)
        h = C.c_void_p()
        _lib.check(_lib.lib().ah_index_insert_items(self._h, _ptr(arr), arr.size, _ptr(seeds), C.byref(h)))
        return self._take_delta(h)

    def graft(self, view, targets, new_index=None, want_map: bool = False) -> Optional[np.ndarray]:
        """ah_index_graft: the trees of `view` (an ah_forest_view: Forest.view_struct() or TreeStore.to_view) join the index,
        tree t in place of the Descendants node targets[t] or, with NEW_ROOT, as a new root.  new_index[k]: the final
        index of view node k (0xFFFFFFFF for a replacing root); None: the new nodes follow the existing ones.  The index is
        renumbered and has no free slots afterwards.  want_map: return the new index of every old node slot."""
        tg = _u32(targets).ravel()
        if tg.size != int(view.n_trees):
            raise ValueError(f"{tg.size} targets for the {int(view.n_trees)} trees of the view")
        ni = None if new_index is None else _u32(new_index).ravel()
        if ni is not None and ni.size != int(view.n_nodes):
            raise ValueError(f"new_index has {ni.size} entries for the {int(view.n_nodes)} nodes of the view")
        out = np.zeros(self.export_info()["n_nodes"], dtype=np.uint32) if want_map else None
        _lib.check(_lib.lib().ah_index_graft(self._h, C.cast(C.byref(view), C.POINTER(_lib.AhForestView)), _ptr(tg), _ptr(ni),
                                             _ptr(out)))
        return out

    def export_info(self) -> dict:
        """ah_index_export_info: n_nodes, desc_len, n_trees, n_normals and the geometry of the normal rows."""
        info = _lib.AhIndexInfo()
        _lib.check(_lib.lib().ah_index_export_info(self._h, C.byref(info)))
        return {f: int(getattr(info, f)) for f, _ in _lib.AhIndexInfo._fields_ if f != "reserved"}

    def export(self, normals: bool = True) -> dict:
        """ah_index_export: the index as it is on the device — nodes (the ah_node record: kind 0 is a free slot, `offset` of a
        split node is its normal row), roots, descendants and, with normals=True, normal_rows (n_normals x row bytes, u8) and
        normal_headers (n_normals x header floats)."""
        info = self.export_info()
        nodes = np.zeros(info["n_nodes"], dtype=_NODE_DT)
        roots = np.zeros(info["n_trees"], dtype=np.uint32)
        desc = np.zeros(info["desc_len"], dtype=np.uint32)
        rows = np.zeros((info["n_normals"], info["normal_row_bytes"]), dtype=np.uint8) if normals else None
        hdrs = np.zeros((info["n_normals"], info["normal_header_floats"]), dtype=np.float32) if normals else None
        _lib.check(_lib.lib().ah_index_export(self._h, _ptr(nodes), _ptr(roots), _ptr(desc), _ptr(rows), _ptr(hdrs)))
        out = {"nodes": nodes, "roots": roots, "descendants": desc}
        if normals:
            out["normal_rows"], out["normal_headers"] = rows, hdrs
        return out

    def encode_nodes(self, indices=None, node_ids=None, base: int = 0, sizes_only: bool = False, out_cap: int | None = None,
                     want_stats: bool = False):
        """ah_index_encode_nodes: the `NodeCodec` values (what LMDB stores) of the node slots `indices` of the index as it is on
        the device, in the order listed; None: of every slot, a free one giving b"".  Children are written as the store's ids:
        node_ids[slot] (one per node slot of the index) or base + slot.  Returns a list of bytes, or with sizes_only the value
        offsets (len + 1, uint64); with want_stats (that, ah_index_encode_stats as a dict)."""
        idx = None if indices is None else _u32(indices).ravel()
        n = self.export_info()["n_nodes"] if idx is None else idx.size
        ids = None if node_ids is None else _u32(node_ids).ravel()
        if ids is not None and ids.size != self.export_info()["n_nodes"]:
            raise ValueError(f"node_ids has {ids.size} entries for the {self.export_info()['n_nodes']} node slots of the index")
        st = _lib.AhIndexEncodeStats()
        ends = np.zeros(n + 1, dtype=np.uint64)
        fn = _lib.lib().ah_index_encode_nodes
        # (an empty list still has a pointer: NULL means every slot)
        held = None if idx is None else (idx if idx.size else np.zeros(1, np.uint32))  # (kept alive across both calls)
        idx_p = None if held is None else held.ctypes.data
        _lib.check(fn(self._h, idx_p, n, _ptr(ids), int(base), None, 0, _ptr(ends), C.byref(st)))
        if not sizes_only:
            cap = int(ends[n]) if out_cap is None else int(out_cap)
            out = np.full(int(ends[n]) + 64, 0xA5, dtype=np.uint8)  # (the tail shows a write past the values)
            try:
                _lib.check(fn(self._h, idx_p, n, _ptr(ids), int(base), _ptr(out), cap, _ptr(ends), C.byref(st)))
            finally:
                assert bool(np.all(out[int(ends[n]):] == 0xA5)), "ah_index_encode_nodes wrote past the end of its values"
        res = ends if sizes_only else [out[int(ends[i]): int(ends[i + 1])].tobytes() for i in range(n)]
        if want_stats:
            return res, {f: (float if f == "seconds" else int)(getattr(st, f)) for f, _ in _lib.AhIndexEncodeStats._fields_}
        return res

    def footprint(self) -> dict:
        """ah_index_footprint_get: node slots and the free ones among them, normal rows in use / live / room for, desc_len and
        the bytes of HBM the index holds (counted on the device; legal with live filters)."""
        fp = _lib.AhIndexFootprint()
        _lib.check(_lib.lib().ah_index_footprint_get(self._h, C.byref(fp)))
        return {f: int(getattr(fp, f)) for f, _ in _lib.AhIndexFootprint._fields_}

    def audit(self, trees: bool = False) -> dict:
        """ah_index_audit: `Reader::assert_validity` of the index as it is on the device, nothing exported.  Returns the
        counts by lower-case class name (_lib.AUDIT_CLASSES), `valid`, n_items / n_trees / nodes_in_use / nodes_reached,
        `first_node` (class -> smallest offending node, BAD_ROOT: position in the roots; None: none) and the first_missing_* /
        first_duplicate_* pairs (None: none); with trees=True also `tree_stats`, one dict per tree in the shape of
        TreeStore.stats plus `root` and `items`.  Reads only; a finding is a result, not an error."""
        rep = _lib.AhIndexAuditReport()
        n_trees = self.export_info()["n_trees"] if trees else 0
        ts = (_lib.AhTreeStats * max(1, n_trees))() if trees else None
        _lib.check(_lib.lib().ah_index_audit(self._h, C.byref(rep), ts))
        return _audit_dict(rep, ts, n_trees if trees else None)

    def tree_stats(self) -> list:
        """`Reader::stats` per tree (src/reader.rs:210-252), counted on the device: audit(trees=True)["tree_stats"]."""
        return self.audit(trees=True)["tree_stats"]

    def compact(self, want_map: bool = False):
        """ah_index_compact: free node slots, orphaned normal rows and spare rows go; the index becomes what a fresh Index of
        the forest as it is now would be, node for node and row for row.  Returns the stats (sizes before / after, `moved`: 0
        when there was nothing to do); with want_map (stats, the new index of every old node slot, 0xFFFFFFFF for a free one)."""
        st = _lib.AhIndexCompactStats()
        out = np.zeros(self.export_info()["n_nodes"], dtype=np.uint32) if want_map else None
        _lib.check(_lib.lib().ah_index_compact(self._h, _ptr(out), C.byref(st)))
        stats = {f: int(getattr(st, f)) for f, _ in _lib.AhIndexCompactStats._fields_ if f != "reserved"}
        return (stats, out) if want_map else stats

    def suspend(self, keep_filters: bool = False) -> None:
        """ah_index_suspend: give up the hold on the dataset, so that Dataset.update_vectors goes through; until resume()
        every search, route, filter or delete call on this index is refused.  The live filters of the index are closed first,
        as close() does (ah_index_suspend refuses while one is alive), or with keep_filters suspended (Filter.suspend), for
        resume_filters once the index is resumed and maintained.  Filters that are suspended already are left alone."""
        for f in list(self._filters):
            if f.suspended:
                continue
            if keep_filters:
                f.suspend()
            else:
                f.close()
        _lib.check(_lib.lib().ah_index_suspend(self._h))

    def resume(self, dataset: Optional[Dataset] = None) -> None:
        """ah_index_resume on the dataset the index was made on (the default), after its update."""
        ds = self.dataset if dataset is None else dataset
        _lib.check(_lib.lib().ah_index_resume(self._h, ds._h))

    def close(self) -> None:
        if self._h:
            for f in list(self._filters):  # (ah_index_destroy refuses while one is alive)
                f.close()
            _lib.lib().ah_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _audit_dict(rep, ts, n_trees) -> dict:
    def some(v):
        return None if int(v) == 0xFFFFFFFF else int(v)
    out = {name: int(rep.count[c]) for c, name in enumerate(_lib.AUDIT_CLASSES)}
    out.update(valid=int(rep.valid), n_items=int(rep.n_items), n_trees=int(rep.n_trees), nodes_in_use=int(rep.nodes_in_use),
               nodes_reached=int(rep.nodes_reached),
               first_node={name: some(rep.first_node[c]) for c, name in enumerate(_lib.AUDIT_CLASSES)})
    # (0xFFFFFFFF is a legal id: whether there is a first pair is said by the count)
    for cls, key in (("missing", "first_missing"), ("duplicate", "first_duplicate")):
        has = out[cls] > 0
        out[key + "_tree"] = int(getattr(rep, key + "_tree")) if has else None
        out[key + "_id"] = int(getattr(rep, key + "_id")) if has else None
    if n_trees is not None:
        out["tree_stats"] = [{"root": int(t.root), "depth": int(t.depth), "split_nodes": int(t.split_nodes),
                              "dummy_normals": int(t.dummy_normals), "descendants": int(t.descendants), "items": int(t.items)}
                             for t in ts[:n_trees]]
    return out


def audit_view(ds: Dataset, view, trees: bool = False) -> dict:
    """ah_forest_view_audit: Index.audit of arrays the host holds (an ah_forest_view: Forest.view_struct() or
    TreeStore.to_view), without making an index of them.  What Index(ds, None, view=view) would refuse is counted."""
    rep = _lib.AhIndexAuditReport()
    n_trees = int(view.n_trees)
    ts = (_lib.AhTreeStats * max(1, n_trees))() if trees else None
    _lib.check(_lib.lib().ah_forest_view_audit(ds._h, C.cast(C.byref(view), C.POINTER(_lib.AhForestView)), C.byref(rep), ts))
    return _audit_dict(rep, ts, n_trees if trees else None)


def audit_findings(report: dict) -> str:
    """The non-zero classes of an audit report and their first offenders, for an error message ('' when valid)."""
    parts = []
    for name in _lib.AUDIT_CLASSES:
        if report[name]:
            where = f"first at {'root position' if name == 'bad_root' else 'node'} {report['first_node'][name]}"
            if name in ("missing", "duplicate"):
                where = f"first: tree {report['first_' + name + '_tree']}, id {report['first_' + name + '_id']}"
            parts.append(f"{name} {report[name]} ({where})")
    return "; ".join(parts)


class Filter:
    """`QueryBuilder::candidates` resident next to an Index (ah_filter_create): the bitmap over the stored ids and what it keeps of
    every leaf, made once.  Immutable; any number of threads may search under it.  Closed with its index at the latest.
    `a & b`, `a | b`, `a - b` and `~a` make the filter of the expression on the device (Index.combine_filters)."""

    def __init__(self, index: Index, ids, sorted_ids: bool = False):
        self.index = index
        self._h = C.c_void_p()
        arr = _u32(ids) if sorted_ids else _u32(sorted(set(int(c) for c in ids)))
        self._suspended = False
        _lib.check(_lib.lib().ah_filter_create(index._h, _ptr(arr), arr.size, C.byref(self._h)))
        index._filters.add(self)

    @classmethod
    def _adopt(cls, index: Index, handle: C.c_void_p) -> "Filter":
        """A Filter around an ah_filter handle the library has just made (Index.combine_filters, Index.make_filter_bitmap)."""
        self = cls.__new__(cls)
        self.index, self._h, self._suspended = index, handle, False
        index._filters.add(self)
        return self

    def suspend(self) -> None:
        """ah_filter_suspend: the filter keeps its bitmap and stops counting as alive, so that the maintenance calls of its index
        (delete_items, insert_items, graft, drop_trees, compact) and Index.suspend go through; until Index.resume_filters it is
        refused by search, the expressions, export and suspend.  info() and close() stay legal."""
        _lib.check(_lib.lib().ah_filter_suspend(self._handle()))
        self._suspended = True

    @property
    def suspended(self) -> bool:
        return bool(self._h) and self._suspended

    def _handle(self):
        if not self._h:
            raise ValueError("the filter is closed")
        return self._h.value

    def info(self) -> dict:
        """ah_filter_info: ids listed (a combined or bitmap-made filter: bits set), those of them that are stored (exact),
        bytes of HBM held."""
        listed, stored, nbytes = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(_lib.lib().ah_filter_info(self._handle(), C.byref(listed), C.byref(stored), C.byref(nbytes)))
        return {"listed": listed.value, "stored": stored.value, "device_bytes": nbytes.value}

    def kept_total(self) -> int:
        """ah_filter_kept_total: the ids the filter keeps summed over every leaf, duplicates across trees included — what a
        descent that drains its queue collects.  A query whose effective search_k is at least this is exhausted."""
        out = C.c_uint64()
        _lib.check(_lib.lib().ah_filter_kept_total(self._handle(), C.byref(out)))
        return int(out.value)

    def kept_ids(self) -> np.ndarray:
        """ah_filter_kept_ids (test aid): the ascending distinct ids the filter keeps and some leaf holds; makes the list on the
        device if it does not exist yet."""
        n = C.c_uint64()
        _lib.check(_lib.lib().ah_filter_kept_ids(self._handle(), None, 0, C.byref(n)))
        ids = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            _lib.check(_lib.lib().ah_filter_kept_ids(self._handle(), _ptr(ids), n.value, C.byref(n)))
        return ids

    def export(self) -> dict:
        """ah_filter_export (test aid): len_bits (largest stored id + 1), bits (its ceil(len_bits / 32) bitmap words) and
        leaf_kept (per node slot of the index: the ids of the leaf the filter keeps), read back from the device."""
        len_bits = C.c_uint64()
        _lib.check(_lib.lib().ah_filter_export(self._handle(), C.byref(len_bits), None, None))
        bits = np.zeros((len_bits.value + 31) // 32, dtype=np.uint32)
        kept = np.zeros(self.index.export_info()["n_nodes"], dtype=np.uint32)
        _lib.check(_lib.lib().ah_filter_export(self._handle(), None, _ptr(bits), _ptr(kept)))
        return {"len_bits": int(len_bits.value), "bits": bits, "leaf_kept": kept}

    def __and__(self, other: "Filter") -> "Filter":
        return self.index.combine_filters("and", [self, other])

    def __or__(self, other: "Filter") -> "Filter":
        return self.index.combine_filters("or", [self, other])

    def __sub__(self, other: "Filter") -> "Filter":
        return self.index.combine_filters("andnot", [self, other])

    def __invert__(self) -> "Filter":
        return self.index.combine_filters("not", [self])

    def close(self) -> None:
        if self._h:
            _lib.lib().ah_filter_destroy(self._h)
            self._h = C.c_void_p()
            self.index._filters.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamedForest:
    """What a sink of ah_build_forest_stream has seen, kept as dictionaries (test aid: small forests)."""

    def __init__(self, distance, dimensions, node_id_base: int = 0):
        self.distance, self.dimensions, self.node_id_base = distance, dimensions, node_id_base
        self.splits, self.leaves, self.roots = {}, {}, None
        self.batches = []  # (kind, level, n_nodes, payload_len) in arrival order
        self.values = {}   # encoded batches: node id (minus the base) -> the value's bytes as they arrived

    def _take_encoded(self, b, payload) -> int:
        """A batch of NodeCodec values (normal_stride == 0): the same dictionaries, ids minus node_id_base."""
        from . import node_codec
        n, base = int(b.n_nodes), self.node_id_base
        for i in range(n):
            nd = b.nodes[i]
            assert nd.kind == b.kind, f"node {nd.id} of kind {nd.kind} in a batch of kind {b.kind}"
            nid = int(nd.id) - base
            assert nid >= 0 and nid not in self.splits and nid not in self.leaves, f"node {nd.id} arrives twice or lies below the base"
            lo = int(nd.payload_offset)
            hi = int(b.nodes[i + 1].payload_offset) if i + 1 < n else int(b.payload_len)
            value = payload[lo:hi].tobytes()
            self.values[nid] = value
            dec = node_codec.decode_value(self.distance, self.dimensions, value)
            if nd.kind == 2:
                assert dec[0] == "S" and (dec[1], dec[2]) == (int(nd.left), int(nd.right)), (nd.id, dec[:3], nd.left, nd.right)
                assert (dec[3] is not None) == bool(nd.has_normal), nd.id
                self.splits[nid] = (dec[3], dec[1] - base, dec[2] - base, int(nd.tree), int(nd.depth), int(nd.count))
            else:
                assert dec[0] == "D" and dec[1].size == int(nd.count), (nd.id, dec[1].size, nd.count)
                self.leaves[nid] = (tuple(int(x) for x in dec[1]), int(nd.tree), int(nd.depth))
        return 0

    def take(self, b) -> int:
        n = int(b.n_nodes)
        self.batches.append((int(b.kind), int(b.level), n, int(b.payload_len)))
        payload = np.ctypeslib.as_array(b.payload, shape=(int(b.payload_len),)) if b.payload_len else np.zeros(0, np.uint8)
        if int(b.normal_stride) == 0 and int(b.normal_vector_offset) == 0 and int(b.normal_header_offset) == 0:
            return self._take_encoded(b, payload)
        hs, vs = self.distance.header_size(), self.distance.vector_size(self.dimensions)
        for i in range(n):
            nd = b.nodes[i]
            assert nd.kind == b.kind, f"node {nd.id} of kind {nd.kind} in a batch of kind {b.kind}"
            assert nd.id not in self.splits and nd.id not in self.leaves, \
                f"node {nd.id} (kind {nd.kind}, tree {nd.tree}, depth {nd.depth}, count {nd.count}) arrives twice; batches so far {self.batches[-6:]}"
            off = int(nd.payload_offset)
            if nd.kind == 2:
                nb = None
                if nd.has_normal:
                    rec = payload[off: off + int(b.normal_stride)]
                    h = rec[int(b.normal_header_offset): int(b.normal_header_offset) + hs]
                    v = rec[int(b.normal_vector_offset): int(b.normal_vector_offset) + vs]
                    nb = h.tobytes() + v.tobytes()  # the canonical form of Forest.canonical / the oracle: [header][vector]
                self.splits[int(nd.id)] = (nb, int(nd.left), int(nd.right), int(nd.tree), int(nd.depth), int(nd.count))
            else:
                ids = payload[off: off + 4 * int(nd.count)].view(np.uint32)
                self.leaves[int(nd.id)] = (tuple(int(x) for x in ids), int(nd.tree), int(nd.depth))
        return 0

    def canonical(self, tree: int):
        import sys
        sys.setrecursionlimit(100000)

        def rec(i):
            if i in self.leaves:
                return ("D", self.leaves[i][0])
            nb, left, right = self.splits[i][:3]
            return ("S", nb, rec(left), rec(right))
        return rec(int(self.roots[tree]))


class Forest:
    """Host-side result of one forest build (ah_forest): flat nodes, normals blob, descendant ids."""

    def __init__(self, handle: C.c_void_p, distance: type[Distance], dimensions: int):
        self._h = handle
        self.distance = distance
        self.dimensions = dimensions
        v = _lib.AhForestView()
        _lib.check(_lib.lib().ah_forest_view_get(self._h, C.byref(v)))
        self.n_trees = int(v.n_trees)
        n = int(v.n_nodes)
        node_dt = np.dtype([("kind", "u1"), ("has_normal", "u1"), ("reserved", "<u2"), ("tree", "<u4"), ("left", "<u4"),
                            ("right", "<u4"), ("offset", "<u8"), ("count", "<u4"), ("depth", "<u4")], align=True)
        assert node_dt.itemsize == C.sizeof(_lib.AhNode)

        def view(ptr, count, dtype):
            # zero-copy numpy view of a buffer owned by the ah_forest handle (kept alive by self)
            if not count:
                return np.zeros(0, dtype)
            nbytes = count * np.dtype(dtype).itemsize
            buf = (C.c_uint8 * nbytes).from_address(C.cast(ptr, C.c_void_p).value)
            return np.frombuffer(buf, dtype=dtype, count=count)

        self.roots = view(v.roots, self.n_trees, np.uint32)
        self.nodes = view(v.nodes, n, node_dt)
        self.normal_stride = int(v.normal_stride)
        self._vec_off, self._hdr_off = int(v.normal_vector_offset), int(v.normal_header_offset)
        self.normals = view(v.normals, int(v.normals_len), np.uint8)
        self.descendants = view(v.descendants, int(v.descendants_len), np.uint32)
        st = _lib.AhBuildStats()
        _lib.check(_lib.lib().ah_forest_stats(self._h, C.byref(st)))
        self.stats = {f: getattr(st, f) for f, _ in _lib.AhBuildStats._fields_}
        self.stats["margin_mode_launches"] = list(st.margin_mode_launches)

    def view_struct(self) -> "_lib.AhForestView":
        """The ah_forest_view of this forest (pointers into the handle's own buffers: valid while the forest lives) — what
        `Index(ds, None, view=...)` / ah_index_create_from_view takes."""
        v = _lib.AhForestView()
        _lib.check(_lib.lib().ah_forest_view_get(self._h, C.byref(v)))
        return v

    @property
    def resident(self) -> bool:
        """The forest holds its device copy (ah_forest_resident_info): built with resident=True, and neither released nor
        consumed by Index.from_forest / Index.graft_forest since."""
        r = C.c_int(0)
        _lib.check(_lib.lib().ah_forest_resident_info(self._h, C.byref(r), None))
        return bool(r.value)

    @property
    def device_bytes(self) -> int:
        b = C.c_uint64(0)
        _lib.check(_lib.lib().ah_forest_resident_info(self._h, None, C.byref(b)))
        return int(b.value)

    def release_device(self) -> None:
        """ah_forest_release_device: give the device copy back; the forest stays, as an ordinary one."""
        _lib.check(_lib.lib().ah_forest_release_device(self._h))

    def digest(self):
        """(total, per-tree array) 64-bit content digests (ah_forest_digest): equal for equal forests whatever the
        margin mode, tuning or batching that built them."""
        per = np.zeros(self.n_trees, dtype=np.uint64)
        total = C.c_uint64(0)
        _lib.check(_lib.lib().ah_forest_digest(self._h, _ptr(per), C.byref(total)))
        return int(total.value), per

    def digest_keyed(self, tree_keys: Sequence[int]) -> np.ndarray:
        """Per-tree digests with `tree_keys[t]` in place of the tree's index inside this forest (ah_forest_digest_keyed): the
        digest of a tree is then the same whichever share / device built it."""
        keys = np.ascontiguousarray(tree_keys, dtype=np.uint64)
        assert keys.size == self.n_trees
        per = np.zeros(self.n_trees, dtype=np.uint64)
        _lib.check(_lib.lib().ah_forest_digest_keyed(self._h, _ptr(keys), _ptr(per)))
        return per

    def close(self) -> None:
        if self._h:
            self.roots = self.nodes = self.normals = self.descendants = None
            _lib.lib().ah_forest_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def normal_of(self, node: int):
        """(header f32[], vector codec bytes) of a split node, or None for `normal: None`."""
        nd = self.nodes[node]
        if nd["kind"] != 2 or not nd["has_normal"]:
            return None
        hs, vs = self.distance.header_size(), self.distance.vector_size(self.dimensions)
        raw = self.normals[int(nd["offset"]): int(nd["offset"]) + self.normal_stride]
        return (raw[self._hdr_off: self._hdr_off + hs].view(np.float32).copy(),
                raw[self._vec_off: self._vec_off + vs].copy())

    def descendants_of(self, node: int) -> np.ndarray:
        nd = self.nodes[node]
        return self.descendants[int(nd["offset"]): int(nd["offset"]) + int(nd["count"])]

    def canonical(self, tree: int):
        """Numbering-independent nested tuples; comparable with oracle.Tree.canonical()."""
        import sys
        sys.setrecursionlimit(100000)

        def rec(i):
            nd = self.nodes[i]
            if nd["kind"] == 1:
                return ("D", tuple(int(x) for x in self.descendants_of(i)))
            nb = None
            if nd["has_normal"]:
                h, v = self.normal_of(i)  # canonical form = [header][vector], the oracle's record layout
                nb = h.tobytes() + v.tobytes()
            return ("S", nb, rec(int(nd["left"])), rec(int(nd["right"])))

        return rec(int(self.roots[tree]))

    def tree_stats(self, tree: int):
        """`Reader::stats` per tree (src/reader.rs:210-252): depth, split nodes, dummy normals, descendants."""
        depth = splits = dummies = descs = 0
        stack = [(int(self.roots[tree]), 1)]
        while stack:
            i, d = stack.pop()
            nd = self.nodes[i]
            depth = max(depth, d)
            if nd["kind"] == 1:
                descs += 1
            else:
                splits += 1
                dummies += 0 if nd["has_normal"] else 1
                stack.append((int(nd["left"]), d + 1))
                stack.append((int(nd["right"]), d + 1))
        return {"depth": depth, "split_nodes": splits, "dummy_normals": dummies, "descendants": descs}
