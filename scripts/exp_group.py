"""Staging a 10M x 768 dataset for a multi-device build, three ways, and a 100-tree build on a device group:

  plain      Dataset.upload_vectors (one replica)
  group      DatasetGroup.upload_vectors on the devices given (default [0, 0]: two replicas on one GPU) — every chunk is
             gathered from the caller's array once and sent to every member from the same pinned slot
  replicate  Dataset.upload_vectors + ah_dataset_replicate onto the group's other devices (a device-to-device copy each)

then the 100-tree forest (the seeds bench.py uses) streamed from the plain dataset (ah_build_forest_stream) and from the group
(ah_build_forest_group_stream), compared through a digest of the stream that does not depend on node numbering or arrival
order: per tree, the sum of a hash over every node's (kind, depth, count, payload bytes).  The same content digest of the
plain dataset's materialised forest (ah_build_forest) ties both streams to that forest's `union` digest — the per-tree
ah_forest_digest_keyed values folded as bench.py folds them (e508e3c6fa7e86f1 for 10M x 768 at seed 42).

Host gather seconds (AH_TIMING's upload lines: the copy out of the caller's array into the pinned ring) are reported next to
the whole-call seconds: a group gathers once whatever the number of members.

    python scripts/exp_group.py [--n 10000000] [--devices 0,0] [--trees 100]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arroy_amd import Dataset, DatasetGroup, _lib, distances, shard  # noqa: E402

SEED, DIMS = 42, 768
MASK = (1 << 64) - 1


class StreamDigest:
    """Per tree: sum mod 2^64 of one 64-bit hash per node (numbering- and order-independent), computed batch by batch."""

    def __init__(self, n_trees):
        self.per_tree = np.zeros(n_trees, dtype=np.uint64)
        self.nodes = 0
        self.w = None

    def _weights(self, n):
        if self.w is None or self.w.size < n:
            self.w = np.random.default_rng(7).integers(1, 1 << 62, size=max(n, 4096), dtype=np.uint64) | np.uint64(1)
        return self.w[:n]

    def _finish(self, tree, kind, count, depth, h):
        with np.errstate(over="ignore"):
            h = h * np.uint64(0xD6E8FEB86659FD93) + kind.astype(np.uint64) * np.uint64(0x100000001B3) + depth.astype(
                np.uint64) * np.uint64(0xBF58476D1CE4E5B9) + count.astype(np.uint64) * np.uint64(0x94D049BB133111EB)
            h ^= h >> np.uint64(29)
            np.add.at(self.per_tree, tree.astype(np.int64), h)
        self.nodes += int(tree.size)

    def _rows_hash(self, words):
        with np.errstate(over="ignore"):
            return (words.astype(np.uint64) * self._weights(words.shape[1])[None, :]).sum(axis=1, dtype=np.uint64)

    def take_forest(self, forest):
        """The same digest over a materialised ah_forest (nodes in any order: the digest is a per-tree sum)."""
        nodes, stride = forest.nodes, int(forest.normal_stride)
        with np.errstate(over="ignore"):
            ids = forest.descendants.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            cs = np.zeros(ids.size + 1, dtype=np.uint64)
            np.cumsum(ids, dtype=np.uint64, out=cs[1:])
            del ids
        step = 16384
        for lo in range(0, len(nodes), step):
            nd = nodes[lo: lo + step]
            kind, has = nd["kind"].astype(np.uint64), nd["has_normal"] != 0
            off, count = nd["offset"].astype(np.int64), nd["count"].astype(np.int64)
            h = np.zeros(len(nd), dtype=np.uint64)
            split = (nd["kind"] == 2) & has
            if split.any():
                idx = np.nonzero(split)[0]
                rows = forest.normals[off[idx][:, None] + np.arange(stride, dtype=np.int64)[None, :]]
                h[idx] = self._rows_hash(rows.view(np.uint32).reshape(idx.size, stride // 4))
            leaf = nd["kind"] == 1
            if leaf.any():
                with np.errstate(over="ignore"):
                    h[leaf] = cs[off[leaf] + count[leaf]] - cs[off[leaf]]
            self._finish(nd["tree"], kind, nd["count"], nd["depth"], h)
        return self

    def take(self, b) -> int:
        n = int(b.n_nodes)
        if not n:
            return 0
        raw = np.frombuffer(np.ctypeslib.as_array(C_u8(b.nodes), shape=(n * 40,)).tobytes(), dtype=np.uint32).reshape(n, 10)
        tree, kind_bits, count, depth, off = raw[:, 1], raw[:, 2], raw[:, 5], raw[:, 6], raw[:, 8].astype(np.uint64)
        kind = (kind_bits & 0xFF).astype(np.uint64)
        payload = np.ctypeslib.as_array(b.payload, shape=(int(b.payload_len),)) if b.payload_len else np.zeros(0, np.uint8)
        h = np.zeros(n, dtype=np.uint64)
        with np.errstate(over="ignore"):
            if int(b.kind) == 2:
                stride = int(b.normal_stride)
                has = ((kind_bits >> 8) & 0xFF) != 0
                if has.any():
                    words = np.zeros((n, stride // 4), dtype=np.uint32)
                    idx = np.nonzero(has)[0]
                    rows = payload[(off[idx][:, None] + np.arange(stride, dtype=np.uint64)[None, :]).astype(np.int64)]
                    words[idx] = rows.view(np.uint32).reshape(idx.size, stride // 4)
                    h = self._rows_hash(words)
            else:
                ids = payload.view(np.uint32).astype(np.uint64)
                starts = (off // 4).astype(np.int64)
                nz = count > 0
                sums = np.zeros(n, dtype=np.uint64)
                if nz.any():
                    sums[nz] = np.add.reduceat(ids * np.uint64(0x9E3779B97F4A7C15), starts[nz], dtype=np.uint64)
                h = sums
        self._finish(tree, kind, count, depth, h)
        return 0

    def total(self):
        x = 0
        for t, v in enumerate(self.per_tree.tolist()):
            x = (x * 0x100000001B3 + v + t) & MASK
        return f"{x:016x}"


def C_u8(p):
    import ctypes
    return ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8))


def union_digest(per_tree):
    """bench.py's fold of the per-tree keyed digests (tree index -> ah_forest_digest_keyed) into one value."""
    h = 0xCBF29CE484222325
    for t in sorted(per_tree):
        h = ((h ^ (int(per_tree[t]) & MASK)) * 0x100000001B3 + t) & MASK
    return h


def gather_seconds(fn):
    """Run fn with AH_TIMING=1 and the library's stderr captured; returns the summed `gather` seconds of its upload lines."""
    import re
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            with _lib.tuning(AH_TIMING=1):
                fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode("utf-8", "replace")
    return round(sum(float(x) for x in re.findall(r"upload_vectors .*?gather ([0-9.]+) s", text)), 4)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--devices", default="0,0")
    ap.add_argument("--trees", type=int, default=100)
    args = ap.parse_args()
    n, devices = args.n, [int(d) for d in args.devices.split(",")]
    ids = np.arange(n, dtype=np.uint32)
    rows = np.empty((n, DIMS), dtype=np.float32)
    chunk = 1 << 20
    for lo in range(0, n, chunk):
        _lib.synth_rows_host(SEED, 1, min(chunk, n - lo), DIMS, first_item=lo, out=rows[lo: lo + chunk])
    seeds = shard.tree_seeds(SEED, range(args.trees))
    res = {"n": n, "dims": DIMS, "devices": devices, "trees": args.trees}

    # plain: one dataset; its streamed forest is the reference
    ds = Dataset(distances.Cosine, DIMS, n)
    res["plain_gather_s"] = gather_seconds(lambda: res.__setitem__("plain_upload_s", timed(lambda: ds.upload_vectors(ids, rows))[1]))
    _, res["plain_finalize_s"] = timed(ds.finalize)
    ref = StreamDigest(args.trees)
    (_r, st, _c), res["plain_build_s"] = timed(lambda: ds.build_forest_stream(seeds, sink=ref.take))
    res["plain_build_device_s"] = round(st["seconds_device"], 4)
    # the materialised forest of the same seeds: bench.py's union digest, and the stream digest of its content
    forest = ds.build_forest(seeds)
    res["forest_union_digest"] = f"{union_digest(dict(zip(range(args.trees), forest.digest_keyed(list(range(args.trees)))))):016x}"
    res["forest_stream_digest"] = StreamDigest(args.trees).take_forest(forest).total()
    forest.close()
    ds.close()

    # stage + ah_dataset_replicate onto the other devices
    src = Dataset(distances.Cosine, DIMS, n, device=devices[0])
    res["replicate_gather_s"] = gather_seconds(
        lambda: res.__setitem__("replicate_upload_s", timed(lambda: src.upload_vectors(ids, rows))[1]))
    reps, res["replicate_copy_s"] = timed(lambda: [src.replicate(d) for d in devices[1:]])
    _, res["replicate_finalize_s"] = timed(lambda: [d.finalize() for d in [src] + reps])
    for r in reps:
        r.close()
    src.close()

    # the group: one host pass, every member fed from the same pinned slot
    g = DatasetGroup(distances.Cosine, DIMS, n, devices)
    res["group_gather_s"] = gather_seconds(lambda: res.__setitem__("group_upload_s", timed(lambda: g.upload_vectors(ids, rows))[1]))
    _, res["group_finalize_s"] = timed(g.finalize)
    got = StreamDigest(args.trees)
    (_r, gst, per, _c), res["group_build_s"] = timed(lambda: g.build_stream(seeds, sink=got.take))
    res["group_build_member_device_s"] = [round(p["seconds_device"], 4) for p in per]
    g.close()

    res["stream_digest_plain"] = ref.total()
    res["stream_digest_group"] = got.total()
    res["nodes_plain"], res["nodes_group"] = ref.nodes, got.nodes
    res["identical"] = bool(ref.total() == got.total() and np.array_equal(ref.per_tree, got.per_tree))
    res["stream_equals_forest"] = res["forest_stream_digest"] == res["stream_digest_plain"]
    for k, v in list(res.items()):
        if isinstance(v, float):
            res[k] = round(v, 4)
    print(json.dumps(res), flush=True)
    return 0 if res["identical"] and res["stream_equals_forest"] else 6


if __name__ == "__main__":
    sys.exit(main())
