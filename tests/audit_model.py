"""Not a test: the model of ah_index_audit / ah_forest_view_audit and the builder of its cases.

`model` restates the class definitions of include/arroy_hip.h ("Audit of a resident index") in plain Python over the arrays of
`Index.export()` or of a view, one sequential walk; it returns the dict `Index.audit` / `audit_view` return, so a test is
`device report == model report`.  `Case` builds a tiny forest from a nested spec as RAW ah_node arrays, which a test may then
break in ways no TreeStore can express (a child out of range, a bad kind, a cycle)."""
import ctypes as C

import numpy as np

from arroy_amd import _lib
from arroy_amd.dataset import _NODE_DT
from arroy_amd.index import TreeStore

NONE = 0xFFFFFFFF
CLASSES = _lib.AUDIT_CLASSES
STRUCTURE = _lib.AUDIT_STRUCTURE
# what is promised when a structure count is non-zero
STRUCTURE_KEYS = ("valid", "n_items", "n_trees", "nodes_in_use", "nodes_reached") + STRUCTURE


def model(nodes, roots, desc, stored_ids, n_normals=None, normals=None, trees=False):
    """nodes: structured array with kind / has_normal / left / right / offset / count (export: a split node's `offset` is its
    normal row and n_normals the rows; view: `offset` is a byte offset and normals = (normals_len, stride)).  roots, desc:
    integer sequences.  stored_ids: the ids of the dataset, ascending (row r holds stored_ids[r])."""
    n_nodes, n_trees = len(nodes), len(roots)
    desc_len = len(desc)
    row_of = {int(i): r for r, i in enumerate(stored_ids)}
    kind = [int(k) for k in nodes["kind"]]
    in_use = [k in (1, 2) for k in kind]
    count = dict.fromkeys(CLASSES, 0)
    first = dict.fromkeys(CLASSES, None)

    def note(cls, where, n=1):
        count[cls] += n
        first[cls] = where if first[cls] is None else min(first[cls], where)

    def valid(i):
        return 0 <= i < n_nodes and in_use[i]
    owner, links = [0] * n_nodes, [0] * n_nodes
    depth = [0] * n_trees
    frontier = []
    for t, r in enumerate(int(r) for r in roots):
        if not valid(r):
            note("bad_root", t)
            continue
        links[r] += 1
        if owner[r] == 0:
            owner[r] = t + 1
            frontier.append(r)
    level = 1
    while frontier:  # every node enters a frontier at most once
        nxt = []
        for i in frontier:
            depth[owner[i] - 1] = level
            if kind[i] != 2:
                continue
            for c in (int(nodes["left"][i]), int(nodes["right"][i])):
                if not valid(c):
                    note("bad_link", i)
                    continue
                links[c] += 1
                if owner[c] == 0:
                    owner[c] = owner[i]
                    nxt.append(c)
        frontier, level = nxt, level + 1
    stats = [{"root": int(r), "depth": depth[t], "split_nodes": 0, "dummy_normals": 0, "descendants": 0, "items": 0}
             for t, r in enumerate(roots)]
    cover = [dict() for _ in range(n_trees)]  # per tree: stored id -> occurrences
    for i in range(n_nodes):
        if links[i] > 1:
            note("linked_twice", i, links[i] - 1)
        if in_use[i] and not owner[i]:
            note("floating", i)
        if not owner[i]:
            continue
        ts, off, cnt = stats[owner[i] - 1], int(nodes["offset"][i]), int(nodes["count"][i])
        if kind[i] == 2:
            ts["split_nodes"] += 1
            if not nodes["has_normal"][i]:
                ts["dummy_normals"] += 1
            elif (off >= n_normals) if normals is None else (off % 4 != 0 or off + normals[1] > normals[0]):
                note("bad_normal", i)
            continue
        ts["descendants"] += 1
        if off + cnt > desc_len:
            note("bad_list", i)
            continue
        ts["items"] += cnt
        ids = [int(x) for x in desc[off:off + cnt]]
        if any(a >= b for a, b in zip(ids, ids[1:])):
            note("unsorted", i)
        for x in ids:
            if x not in row_of:
                note("foreign", i)
            else:
                cover[owner[i] - 1][x] = cover[owner[i] - 1].get(x, 0) + 1
    out = {"n_items": len(row_of), "n_trees": n_trees, "nodes_in_use": sum(in_use), "nodes_reached": sum(1 for o in owner if o)}
    pairs = {"duplicate": [], "missing": []}
    for t in range(n_trees):
        pairs["duplicate"] += [(t, x, n - 1) for x, n in cover[t].items() if n > 1]
        pairs["missing"] += [(t, x, 1) for x in row_of if x not in cover[t]]
    for cls, key in (("missing", "first_missing"), ("duplicate", "first_duplicate")):
        count[cls] = sum(p[2] for p in pairs[cls])
        t, x = min(pairs[cls])[:2] if pairs[cls] else (None, None)
        out[key + "_tree"], out[key + "_id"] = t, x
        first[cls] = None if t is None else int(roots[t])  # the root of the first pair's tree
    out.update(count)
    out["first_node"] = first
    out["valid"] = int(not any(count.values()))
    if trees:
        out["tree_stats"] = stats
    return out


def model_of_export(ex, stored_ids, n_normals, trees=False):
    return model(ex["nodes"], ex["roots"], ex["descendants"], stored_ids, n_normals=n_normals, trees=trees)


def structure_part(report):
    """The fields promised whatever the structure: valid, the sizes, the structure counts and their first offenders (and
    every tree's root)."""
    out = {k: report[k] for k in STRUCTURE_KEYS}
    out["first_node"] = {k: report["first_node"][k] for k in STRUCTURE}
    if "tree_stats" in report:
        out["roots"] = [t["root"] for t in report["tree_stats"]]
    return out


def reference_valid(nodes, roots, desc, stored_ids):
    """`Reader::assert_validity` with `gather_items_and_tree_ids` (src/reader.rs:509-589), literally, over the arrays of a
    view: True when it passes, False when one of its assertions or look-ups fails.  Lists are RoaringBitmaps there, so an
    order or a repetition inside ONE list is not expressible; a cycle does not terminate there and is not passed here."""
    n = len(nodes)
    tree_ids = {i for i in range(n) if int(nodes["kind"][i]) in (1, 2)}
    item_ids = set(int(i) for i in stored_ids)

    def gather(i):
        if not (0 <= i < n) or int(nodes["kind"][i]) not in (1, 2):
            raise AssertionError(f"Could not find {i}")
        if nodes["kind"][i] == 1:
            off, cnt = int(nodes["offset"][i]), int(nodes["count"][i])
            return {i}, set(int(x) for x in desc[off:off + cnt])
        left, right = gather(int(nodes["left"][i])), gather(int(nodes["right"][i]))
        trees, items = left[0] | right[0], left[1] | right[1]
        assert len(left[0]) + len(right[0]) == len(trees)
        assert len(left[1]) + len(right[1]) == len(items)
        trees.add(i)
        return trees, items
    try:
        for r in roots:
            trees, items = gather(int(r))
            assert item_ids == items, "A tree cannot access to all items"
            assert tree_ids >= trees, "A tree contains an invalid tree node"
            tree_ids -= trees
        assert not tree_ids, "tree nodes floating around"
    except AssertionError:
        return False
    return True


class Case:
    """A forest as raw arrays.  A spec is a list of ids (a Descendants node: the ids exactly as given, not sorted), a pair
    (left, right) (a split node with a normal) or a triple (left, right, None) (a split node with `normal: None`).  Children
    are numbered before their parents; `trees` become roots, `loose` are built the same way and named by no root."""

    def __init__(self, trees, loose=(), stride=64):
        self.stride = stride
        self._nodes, self._desc, self.n_normals = [], [], 0
        self.roots = np.array([self.add(spec) for spec in trees], dtype=np.uint32)
        self.loose = [self.add(spec) for spec in loose]
        self.nodes = np.zeros(len(self._nodes), dtype=_NODE_DT)
        for i, nd in enumerate(self._nodes):
            for f, v in nd.items():
                self.nodes[f][i] = v
        self.desc = np.array(self._desc, dtype=np.uint32)
        self.normals_len = self.n_normals * stride

    def add(self, spec):
        if isinstance(spec, tuple):
            left, right = self.add(spec[0]), self.add(spec[1])
            has = len(spec) == 2
            nd = {"kind": 2, "has_normal": int(has), "left": left, "right": right, "offset": self.n_normals * self.stride if has else 0}
            self.n_normals += int(has)
        else:
            nd = {"kind": 1, "offset": len(self._desc), "count": len(spec)}
            self._desc += [int(x) for x in spec]
        self._nodes.append(nd)
        return len(self._nodes) - 1

    def view(self, dist, dims):
        """-> (ah_forest_view over this case's arrays, keep-alive).  The records are zeros: [header][vector], padded to stride."""
        hs, vs = dist.header_size(), dist.vector_size(dims)
        assert hs + vs <= self.stride and self.stride % 4 == 0
        blob = np.zeros(max(1, self.normals_len), dtype=np.uint8)
        roots = self.roots if self.roots.size else np.zeros(1, np.uint32)
        desc = self.desc if self.desc.size else np.zeros(1, np.uint32)
        nodes = self.nodes if self.nodes.size else np.zeros(1, _NODE_DT)
        v = _lib.AhForestView()
        v.n_trees, v.n_nodes = self.roots.size, self.nodes.size
        v.roots = roots.ctypes.data_as(C.POINTER(C.c_uint32))
        v.nodes = C.cast(nodes.ctypes.data, C.POINTER(_lib.AhNode))
        v.normals = blob.ctypes.data_as(C.POINTER(C.c_uint8))
        v.normals_len = self.normals_len
        v.normal_stride, v.normal_vector_offset, v.normal_header_offset = self.stride, hs, 0
        v.descendants = desc.ctypes.data_as(C.POINTER(C.c_uint32))
        v.descendants_len = self.desc.size
        return v, (blob, roots, desc, nodes)

    def model(self, stored_ids, trees=False):
        """the model's report of this case as a view"""
        return model(self.nodes, self.roots, self.desc, stored_ids, normals=(self.normals_len, self.stride), trees=trees)

    def store(self, dist=None, dims=0):
        """the case as a TreeStore (node index = store id), for TreeStore.stats and, with a distance, TreeStore.to_view (planes
        of zeros); only for a case whose structure is a forest"""
        hs, vs = (dist.header_size(), dist.vector_size(dims)) if dist is not None else (4, 0)
        s = TreeStore()
        for i, nd in enumerate(self.nodes):
            if nd["kind"] == 1:
                s.nodes[i] = ("D", self.desc[int(nd["offset"]):int(nd["offset"]) + int(nd["count"])].copy())
            else:
                s.nodes[i] = ("S", int(nd["left"]), int(nd["right"]), np.zeros(hs // 4, np.float32), bytes(vs) if nd["has_normal"] else None)
        s.roots = [int(r) for r in self.roots]
        return s


def store_stats(store):
    return [store.stats(r) for r in store.roots]


def plain_stats(report):
    """tree_stats of a report in the shape of TreeStore.stats"""
    return [{k: t[k] for k in ("depth", "split_nodes", "dummy_normals", "descendants")} for t in report["tree_stats"]]


# ---- the catalogue: cases ah_index_create_from_view accepts ---------------------------------------------------------------

def spread(ids, sizes):
    """`ids` cut into consecutive lists of the given sizes (the rest in a last list) and hung into a right-leaning chain"""
    parts, at = [], 0
    for n in sizes:
        parts.append(list(ids[at:at + n]))
        at += n
    parts.append(list(ids[at:]))
    spec = parts[-1]
    for p in reversed(parts[:-1]):
        spec = (p, spec)
    return spec


def chain(ids, depth):
    """a degenerate chain: depth - 1 split nodes, each with one empty leaf, all ids in the last leaf: depth `depth`"""
    spec = list(ids)
    for _ in range(depth - 1):
        spec = ([], spec)
    return spec


def catalogue(ids):
    """name -> Case over the stored ids `ids` (ascending, at least 200 of them unless a case says otherwise)"""
    ids = [int(i) for i in ids]
    half = len(ids) // 2
    full = spread(ids, [0, 1, 63, 64, 65])  # lists of 0, 1, 63, 64, 65 ids and the rest
    big = (ids[:130], ids[130:])            # a list of 130 ids
    dummy = (ids[:half], ([], ids[half:]), None)  # `normal: None` above, an empty Descendants node under a split

    def swapped(lst, a, b):
        lst = list(lst)
        lst[a], lst[b] = lst[b], lst[a]
        return lst
    out = {
        "valid": Case([ids, full, dummy, big]),  # (the first root is one Descendants node)
        "missing": Case([full, (ids[:half], ids[half + 1:])]),
        "duplicate": Case([(ids[:half + 1], ids[half:]), full]),
        "duplicate_across_trees": Case([ids, (ids[:half], ids[half:])]),
        # inverted at (63, 64), across the wave's step; an equal pair; inverted at (0, 1)
        "unsorted": Case([(swapped(ids[:130], 63, 64), ids[130:]), (ids[:10] + [ids[9]] + ids[10:half], ids[half:]),
                          (swapped(ids[:half], 0, 1), ids[half:])]),
        "floating": Case([full], loose=[(ids[:3], ids[3:6])]),
        "deep_chain": Case([chain(ids, 40), full]),
        "zero_trees": Case([]),
        "zero_trees_with_nodes": Case([], loose=[(ids[:half], ids[half:]), ids]),
    }
    return out


def foreign_cases(ids, foreign):
    """one tree holding every id plus the foreign ones, each in ascending position; and a valid twin"""
    ids = [int(i) for i in ids]
    merged = sorted(ids + [int(f) for f in foreign])
    half = len(merged) // 2
    return Case([(merged[:half], merged[half:]), ids])


# ---- structures ah_index_create_from_view refuses: through ah_forest_view_audit only ---------------------------------------

def broken(ids):
    """name -> Case, each a valid two-tree forest with one thing broken in its raw arrays"""
    ids = [int(i) for i in ids]
    q = len(ids) // 4
    tree = ((ids[:q], ids[q:2 * q]), (ids[2 * q:3 * q], ids[3 * q:]))  # nodes 0 1 [2] 3 4 [5] [6]; second tree 7 8 [9] 10 11 [12] [13]

    def base():
        return Case([tree, tree])
    out = {}
    c = base()
    c.nodes["left"][12] = 2  # the first tree's left sub-tree under the second tree too
    out["two_parents"] = c
    c = base()
    c.nodes["right"][13] = 6
    out["root_is_a_child"] = c
    c = base()
    c.roots[1] = 6
    out["root_named_twice"] = c
    c = base()
    c.nodes["left"][5] = 5
    out["self_loop"] = c
    c = base()
    c.nodes["right"][9] = 13
    out["cycle_through_an_ancestor"] = c
    c = base()
    c.nodes["right"][2] = 14
    c.nodes["left"][9] = NONE
    out["child_out_of_range"] = c
    c = base()
    c.roots[0] = 14
    out["root_out_of_range"] = c
    c = base()
    c.nodes["kind"][3] = 7
    c.nodes["kind"][8] = 0
    out["bad_kind"] = c
    c = base()
    c.nodes["kind"][13] = 9
    out["bad_kind_root"] = c
    c = base()
    c.nodes["offset"][4] = c.desc.size - 1  # (count >= 2)
    c.nodes["offset"][7] = 1 << 32          # would wrap to 0 in 32 bits
    out["list_beyond_the_blob"] = c
    c = base()
    c.nodes["offset"][6] = c.normals_len      # one record too far
    c.nodes["offset"][9] = c.nodes["offset"][9] + 2  # misaligned
    out["normal_beyond_the_blob"] = c
    return out


# ---- seeded random forests with injected list / coverage faults ----------------------------------------------------------------

def random_case(seed, stored_ids):
    """At most 6 trees and 300 nodes over `stored_ids`, every tree a random split of a random order of the ids down to leaves
    of a random size, then one to three faults: an id taken out of a leaf, an id of the tree added to another leaf, a foreign
    id, two neighbours exchanged, a neighbour repeated."""
    import random
    g = random.Random(seed)
    ids = [int(i) for i in stored_ids]
    have = set(ids)
    foreign = [x for x in range(min(ids), min(ids) + len(ids) + 40) if x not in have]  # (gaps, or just past a dense range)
    n_trees = g.randint(1, 6)
    leaf_max = g.randint(max(8, 2 * len(ids) * n_trees // 140), 64)  # (about 2 n / leaf_max nodes a tree: 300 in all at most)

    def grow(part):
        if len(part) <= leaf_max:
            return sorted(part)
        cut = g.randint(1, len(part) - 1)
        return (grow(part[:cut]), grow(part[cut:])) if g.random() < 0.8 else (grow(part[:cut]), grow(part[cut:]), None)
    specs = [grow(g.sample(ids, len(ids))) for _ in range(n_trees)]

    def leaves(spec, out):
        if isinstance(spec, tuple):
            leaves(spec[0], out)
            leaves(spec[1], out)
        else:
            out.append(spec)
        return out
    for _ in range(g.randint(1, 3)):
        mine = leaves(g.choice(specs), [])
        leaf = g.choice([lf for lf in mine if len(lf) >= 2] or mine)
        what = g.choice(["missing", "duplicate", "foreign", "exchange", "repeat"])
        if what == "missing" and leaf:
            leaf.pop(g.randrange(len(leaf)))
        elif what == "duplicate":
            other = g.choice(mine)
            if other:
                leaf.append(g.choice(other))
                leaf.sort()
        elif what == "foreign":
            leaf.append(g.choice(foreign))
            leaf.sort()
        elif what == "exchange" and len(leaf) >= 2:
            k = g.randrange(len(leaf) - 1)
            leaf[k], leaf[k + 1] = leaf[k + 1], leaf[k]
        elif what == "repeat" and leaf:
            k = g.randrange(len(leaf))
            leaf.insert(k, leaf[k])
    c = Case(specs)
    assert len(c.nodes) <= 300
    return c
