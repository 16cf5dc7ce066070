"""The host side of a forest-build batch (arroy_amd/csrc/forest_records.h: the roots, the digest of a level's node table, the
leaves' merge, the post-order node list, the ring of pending tables, the cuts of the grouped tail, the sizes of a batch's
buffers), checked on the host: a stand-alone program (tests/forest_records_check.cpp, its own main, no device call) built
with AddressSanitizer and UBSan is driven with synthetic forests — random trees of counts, laid out level by level in the
order k_next_emit writes them: by tree, then by parent order, only the children of more than split_after items — and its
printed output is compared with the restatement below, which emits node lists and leaves by plain recursion over the model
trees.  The branches a build only reaches at 10M rows (a digest over several threads, the parent table still pending when
the tail is cut, the ring's wrap and "no room") are reached here with the smallest inputs that do."""
import math
import os
import random
import subprocess

import pytest

from conftest import ROOT
from test_index_workspace_cpu import compilers

SRC = os.path.join(ROOT, "tests", "forest_records_check.cpp")
ST_PENDING, ST_ACCEPTED, ST_RANDOM = 0, 1, 2
DESC, SPLIT = 1, 2
K_TILE = 2048
M64 = (1 << 64) - 1
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("forest_records") / "forest_records_check")
    tried = []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all", "-pthread", SRC, "-o", out], capture_output=True, text=True)
        if build.returncode == 0:
            return out
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))


def run(exe, tmp_path, lines):
    path = tmp_path / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    got = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0 and got.stderr == "", got.stdout[-2000:] + got.stderr[-4000:]
    out = got.stdout.split("\n")
    assert out[-2:] == ["done", ""], out[-3:]
    return out[:-2]


def same(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i}: got {g!r}, expected {w!r}"
    assert len(got) == len(want), f"{len(got)} lines, expected {len(want)}: {(got + want)[min(len(got), len(want))]!r}"


# ---- the model: trees of counts ------------------------------------------------------------------------------------------
def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


class Node:
    def __init__(self, tree, start, count, depth):
        self.tree, self.start, self.count, self.depth = tree, start, count, depth
        self.n_left = self.state = self.attempt = 0
        self.left = self.right = None
        self.rec = None  # record index: handed out in the order the tables are digested
        self.normal_off = 0

    @property
    def split(self):
        return self.left is not None


def grow(rng, tree, start, count, depth, split_after):
    nd = Node(tree, start, count, depth)
    if count <= split_after:
        return nd
    u = rng.random()
    if depth >= 10:
        nd.n_left = count // 2
    elif u < 0.08:
        nd.n_left = 0  # an empty left child
    elif u < 0.16:
        nd.n_left = count  # an empty right child
    else:
        nd.n_left = rng.randint(1, count - 1)
    nd.state = ST_ACCEPTED if rng.random() < 0.7 else ST_RANDOM  # ST_RANDOM: a dummy normal
    nd.attempt = rng.randint(0, 3)
    nd.left = grow(rng, tree, start, nd.n_left, depth + 1, split_after)
    nd.right = grow(rng, tree, start + nd.n_left, count - nd.n_left, depth + 1, split_after)
    return nd


def walk(nd):  # post-order
    if nd.split:
        yield from walk(nd.left)
        yield from walk(nd.right)
    yield nd


def levels_of(roots, split_after):
    level = [r for r in roots if r.count > split_after]
    while level:
        yield level
        level = [c for nd in level for c in (nd.left, nd.right) if c.count > split_after]


class Batch:
    """What the build knows of a batch, and the commands that replay it."""

    def __init__(self, sizes, split_after, seed, first_tree=0, streaming=False, id_base=0, nstride=64, node_base=0, desc_base=0,
                 roots_base=0):
        self.split_after, self.first_tree, self.streaming, self.id_base, self.nstride = split_after, first_tree, streaming, id_base, nstride
        self.node_base, self.desc_base, self.roots_base = node_base, desc_base, roots_base
        rng = random.Random(seed)
        self.bases = [0]
        for c in sizes:
            self.bases.append(self.bases[-1] + c)
        self.seeds = [rng.getrandbits(64) for _ in sizes]
        self.roots = [grow(rng, t, self.bases[t], c, 0, split_after) for t, c in enumerate(sizes)]
        self.n_recs = 0
        self.routed = 0
        self.chunk_off = 1 << 20  # normals of earlier batches
        for r in self.roots:
            r.rec = self.n_recs
            self.n_recs += 1

    def forest_cmd(self):
        n = len(self.roots)
        return [f"forest {n} {self.first_tree} {self.split_after} {int(self.streaming)} {self.id_base} {self.nstride} {self.node_base} "
                f"{self.desc_base} {self.roots_base}", " ".join(map(str, self.bases)), " ".join(map(str, self.seeds))]

    def forest_out(self):
        out, tiles, first = [], 0, [NONE] * (len(self.roots) + 1)
        level = [r for r in self.roots if r.count > self.split_after]
        for i, r in enumerate(level):
            nt = (r.count + K_TILE - 1) // K_TILE
            key = mix64(self.seeds[r.tree] ^ 0xA5A5A5A55A5A5A5A)
            out.append(f"root {i} {key} {r.start} {r.tree} {r.count} 0 0 0 {tiles} {nt} 0")
            first[r.tree] = i
            tiles += nt
        return [f"info {len(level)} {tiles} 0 {sum(r.count for r in level)}"] + out + ["tree_first " + " ".join(map(str, first))]

    def table(self, nodes, threads=1, rec_full=None, fork_parent=False, dump=True):
        """The digest of one table in launch order: the command lines and the expected output."""
        depth, base = nodes[0].depth, self.n_recs
        chunk = self.chunk_off
        self.chunk_off += len(nodes) * self.nstride
        cmd = [f"table {depth} {len(nodes)} {chunk} {int(rec_full is not None)} {rec_full or 0} {threads} {int(fork_parent)} {int(dump)}"]
        sn = []
        for i, nd in enumerate(nodes):
            cmd.append(f"{nd.tree} {nd.start} {nd.count} {nd.n_left} {nd.attempt} {nd.state}")
            nd.normal_off = chunk + i * self.nstride
            nd.left.rec, nd.right.rec = base + 2 * i, base + 2 * i + 1
            left = self.id_base + base + 2 * i
            sn.append(f"sn {self.id_base + nd.rec} {self.first_tree + nd.tree} {SPLIT} {int(nd.state == ST_ACCEPTED)} {left} {left + 1} {nd.count} "
                      f"{depth} {i * self.nstride}")
        self.n_recs += 2 * len(nodes)
        self.routed += sum(nd.count for nd in nodes)
        out = [f"digest {sum((nd.attempt + 1) * nd.count for nd in nodes)} {sum(nd.attempt for nd in nodes)} "
               f"{sum(nd.state != ST_ACCEPTED for nd in nodes)} {sum(nd.count for nd in nodes)} {NONE} n_recs {self.n_recs} routed {self.routed}"]
        if dump:
            if self.streaming:
                out += sn
            kids = [c for nd in nodes for c in (nd.left, nd.right) if c.count > self.split_after]
            out.append(" ".join(["next"] + [str(c.rec) for c in kids]))
        return cmd, out

    def recs_out(self):
        """Every record so far; a node whose table is still to be digested is a split without children or normal."""
        seen = [[nd for nd in walk(r) if nd.rec is not None] for r in self.roots]
        by_rec = {nd.rec: nd for tree in seen for nd in tree}
        assert sorted(by_rec) == list(range(self.n_recs))
        out = []
        for i in range(self.n_recs):
            nd = by_rec[i]
            if nd.split and nd.left.rec is not None:
                out.append(f"rec {i} {SPLIT} {int(nd.state == ST_ACCEPTED)} {nd.tree} {nd.left.rec} {nd.right.rec} {nd.start} {nd.count} {nd.depth} "
                           f"{nd.normal_off}")
            else:
                out.append(f"rec {i} {SPLIT if nd.split else DESC} 0 {nd.tree} 0 0 {nd.start} {nd.count} {nd.depth} 0")
        out.append("tree_count " + " ".join(str(len(tree)) for tree in seen))
        out.append("tree_root " + " ".join(str(r.rec) for r in self.roots))
        return out

    def nodes_out(self, trees=None, mask_offsets=False):
        """The ah_node list by plain recursion: children before parents, forest-local indices."""
        out, roots, counts = [], [], [0, 0]
        at = [self.node_base]

        def emit(nd):
            if nd.split:
                l, r = emit(nd.left), emit(nd.right)
                off = "*" if mask_offsets else nd.normal_off
                line = f"{SPLIT} {int(nd.state == ST_ACCEPTED)} {self.first_tree + nd.tree} {l} {r} {off} {nd.count} {nd.depth}"
            else:
                line = f"{DESC} 0 {self.first_tree + nd.tree} 0 0 {self.desc_base + nd.start} {nd.count} {nd.depth}"
            counts[0 if nd.split else 1] += 1
            out.append(f"node {at[0]} {line}")
            at[0] += 1
            return at[0] - 1

        for r in self.roots if trees is None else self.roots[:trees]:
            roots.append(emit(r))
        return out, roots, counts

    def nodes_dump(self):
        out, roots, counts = self.nodes_out()
        return out + ["roots " + " ".join(map(str, roots)), f"counts {counts[0]} {counts[1]}"]

    def cursor_after(self, trees):
        return self.node_base + sum(1 for r in self.roots[:trees] for _ in walk(r))

    def leaves_out(self, t_a, t_b):
        leaves = [nd for r in self.roots[t_a:t_b] for nd in walk(r) if not nd.split]
        keys = [(nd.tree, nd.start, nd.count) for nd in leaves]
        assert len(set(keys)) == len(keys), "two empty leaves share a start: pick another seed"
        leaves.sort(key=lambda nd: (nd.tree, nd.start, nd.count))  # an empty leaf before the sibling that shares its start
        return [f"leaves {len(leaves)}"] + [f"leaf {self.id_base + nd.rec} {self.first_tree + nd.tree} {DESC} 0 0 0 {nd.count} {nd.depth} {nd.start * 4}"
                                            for nd in leaves]


FIVE = [230, 5, 170, 0, 140]  # one tree that fits its root, one tree of zero items


def five_trees(**kw):
    """The first seed whose forest has what the cases ask for: empty children on either side, dummy normals, attempts 0-3, a
    third level in the first and the last tree, and no two empty leaves at one position (their order would be arbitrary)."""
    for seed in range(1000):
        b = Batch(FIVE, 8, seed, **kw)
        nodes = [nd for r in b.roots for nd in walk(r)]
        splits = [nd for nd in nodes if nd.split]
        leaves = [(nd.tree, nd.start, nd.count) for nd in nodes if not nd.split]
        level2 = {nd.tree for nd in splits if nd.depth == 2}
        if (len(set(leaves)) == len(leaves) and any(nd.n_left == 0 for nd in splits) and any(nd.n_left == nd.count for nd in splits) and
                any(nd.state == ST_RANDOM for nd in splits) and {nd.attempt for nd in splits} == {0, 1, 2, 3} and {0, 4} <= level2 and
                max(nd.depth for nd in splits) >= 4):
            return b
    raise AssertionError("no seed gives the forest the cases need")


def level_by_level(b, threads=1):
    cmd, out = b.forest_cmd(), b.forest_out()
    for level in levels_of(b.roots, b.split_after):
        c, o = b.table(level, threads)
        cmd += c
        out += o
    return cmd, out


# ---- 1: a five-tree batch ---------------------------------------------------------------------------------------------
def test_five_trees_roots_records_and_node_list(exe, tmp_path):
    b = five_trees(node_base=7, desc_base=1000, roots_base=2, nstride=3200)
    cmd, out = level_by_level(b)
    cmd += ["recs", "emit 0 5 1", "nodes"]
    out += b.recs_out() + [f"emit ok cursor {b.cursor_after(5)} tree 5"] + b.nodes_dump()
    # the same forest emitted in three tree ranges; an out-of-order range is refused and changes nothing
    b2 = five_trees(node_base=7, desc_base=1000, roots_base=2, nstride=3200)
    c2, o2 = level_by_level(b2)
    cmd += c2 + ["emit 0 2 1", "emit 3 5 1", "emit 2 2 1", "emit 2 3 2", "emit 3 5 1", "nodes"]
    out += o2 + [f"emit ok cursor {b.cursor_after(2)} tree 2", f"emit refused cursor {b.cursor_after(2)} tree 2",
                 f"emit ok cursor {b.cursor_after(2)} tree 2", f"emit ok cursor {b.cursor_after(3)} tree 3",
                 f"emit ok cursor {b.cursor_after(5)} tree 5"] + b.nodes_dump()
    same(run(exe, tmp_path, cmd), out)


# ---- 2: the same forest, streamed -------------------------------------------------------------------------------------
def test_five_trees_streamed_split_nodes_and_leaves(exe, tmp_path):
    b = five_trees(streaming=True, id_base=1000, first_tree=3, nstride=3200)
    cmd, out = level_by_level(b)
    for t_a, t_b, threads in ((0, 5, 1), (0, 2, 1), (2, 5, 2)):
        cmd.append(f"leaves {t_a} {t_b} {threads}")
        out += b.leaves_out(t_a, t_b)
    # the encoded stream's bound: id_base + the records so far + the two children of every node must not pass 2^32 - 1
    edge = Batch(FIVE, 8, 1, streaming=True, id_base=0xFFFFFFFF - 5 - 20)
    cmd += edge.forest_cmd() + ["wrap 10", "wrap 11"]
    out += edge.forest_out() + ["wrap 0", "wrap 1"]
    same(run(exe, tmp_path, cmd), out)


# ---- 3: one level of 70 000 nodes over 1, 4 and 8 threads --------------------------------------------------------------
def test_a_wide_level_digests_the_same_on_any_number_of_threads(exe, tmp_path):
    n = 70000
    b = Batch([20] * n, 8, 5, streaming=True, id_base=17, first_tree=2, nstride=128)
    level = next(levels_of(b.roots, 8))
    assert len(level) == n
    table, digest = b.table(level)
    forest, roots, recs = b.forest_cmd(), b.forest_out(), b.recs_out()
    with_threads = lambda t, threads: [" ".join(t[0].split()[:6] + [str(threads)] + t[0].split()[7:])] + t[1:]
    cmd, out = [], []
    for threads in (1, 4, 8):  # the same output whatever the number of threads
        cmd += forest + with_threads(table, threads) + ["recs", "grow 10 2 5 6"]
        out += roots + digest + recs + [f"grow {b.n_recs + 2 * (10 + 5 + 6)} n_recs {b.n_recs}"]
    # a node left pending and a node that counted more left items than it has, in different threads' shares: the smallest
    bad = list(table)
    bad[0] = " ".join(bad[0].split()[:9] + ["0"])  # (no dump)
    bad[1 + 60000] = " ".join(bad[1 + 60000].split()[:5] + [str(ST_PENDING)])
    fields = bad[1 + 20000].split()
    bad[1 + 20000] = " ".join(fields[:3] + ["21"] + fields[4:])
    for threads in (1, 4, 8):
        cmd += forest + with_threads(bad, threads)
        out += roots + [f"digest 0 0 0 0 20000 n_recs {3 * n} routed 0"]
    same(run(exe, tmp_path, cmd), out)


# ---- 4 and 5: the grouped tail ------------------------------------------------------------------------------------------
def tail_group_trees(n_trees, groups, ratio_percent):
    k = min(groups, n_trees)
    ratio = min(100, max(10, ratio_percent)) / 100.0
    total_w, w = 0.0, 1.0
    for _ in range(k):
        total_w += w
        w *= ratio
    cut, cum, w = [0] * (k + 1), 0.0, 1.0
    for g in range(1, k):
        cum += w
        at = math.floor(n_trees * cum / total_w + 0.5)  # llround: half away from zero
        cut[g] = min(max(at, cut[g - 1] + 1), n_trees - (k - g))
        w *= ratio
    cut[k] = n_trees
    return cut


def test_tail_group_trees(exe, tmp_path):
    cases = [(n, k, r) for n in (2, 3, 7, 32, 100) for k in (2, 3, 4, 32) for r in (10, 50, 100)]
    want = []
    for n, k, r in cases:
        cut = tail_group_trees(n, k, r)
        assert cut[0] == 0 and cut[-1] == n and len(cut) == min(k, n) + 1 and all(a < b for a, b in zip(cut, cut[1:]))
        want.append("cuts " + " ".join(map(str, cut)))
    same(run(exe, tmp_path, [f"cuts {n} {k} {r}" for n, k, r in cases]), want)


@pytest.mark.parametrize("parent_pending", [False, True])
@pytest.mark.parametrize("streaming", [False, True])
def test_grouped_tail_gives_the_level_by_level_forest(exe, tmp_path, parent_pending, streaming):
    kw = dict(streaming=streaming, id_base=1000 if streaming else 0, first_tree=3 if streaming else 0, nstride=3200, node_base=7, desc_base=1000)
    plain = five_trees(**kw)
    for level in levels_of(plain.roots, 8):
        plain.table(level)
    b = five_trees(**kw)
    levels = list(levels_of(b.roots, 8))
    cut = tail_group_trees(5, 3, 50)
    assert cut == [0, 3, 4, 5]
    cmd, out = b.forest_cmd(), b.forest_out()
    c, o = b.table(levels[0])
    cmd, out = cmd + c, out + o
    # the parent of the cut level: digested before the cut (its children's list swapped at the cut), or still pending then
    # (fork_parent: swapped after its digest)
    c, o = b.table(levels[1], fork_parent=parent_pending)
    cmd, out = cmd + c + ([] if parent_pending else ["swapfull"]), out + o
    for g in range(3):
        trees = range(cut[g], cut[g + 1])
        level = [nd for nd in levels[2] if nd.tree in trees]
        n0 = next((i for i, nd in enumerate(levels[2]) if nd.tree in trees), None)
        first = True
        while level:  # the group to its end: its first table is a slice of the level's, its records level_rec_full[n0 ...]
            c, o = b.table(level, rec_full=n0 if first else None)
            cmd, out = cmd + c, out + o
            level = [k for nd in level for k in (nd.left, nd.right) if k.count > 8]
            first = False
        if streaming:
            cmd.append(f"leaves {cut[g]} {cut[g + 1]} 1")
            out += b.leaves_out(cut[g], cut[g + 1])
            # ... which are the level-by-level run's but for the ids, which follow the order of the digests
            strip = lambda lines: [" ".join(l.split()[2:]) for l in lines[1:]]
            assert strip(b.leaves_out(cut[g], cut[g + 1])) == strip(plain.leaves_out(cut[g], cut[g + 1]))
        else:
            cmd.append(f"emit {cut[g]} {cut[g + 1]} 1")
            out.append(f"emit ok cursor {b.cursor_after(cut[g + 1])} tree {cut[g + 1]}")
    if not streaming:
        cmd.append("nodes")
        out += b.nodes_dump()
        # node for node the level-by-level forest: only normal_off follows the launch order
        assert b.nodes_out(mask_offsets=True) == plain.nodes_out(mask_offsets=True)
        assert b.nodes_out() != plain.nodes_out()
    same(run(exe, tmp_path, cmd), out)


# ---- 6: the ring of pending tables ------------------------------------------------------------------------------------
def test_table_ring_against_a_fifo_model(exe, tmp_path):
    rng = random.Random(11)
    cap = 64 * 4096
    live, head = [], 0  # (offset, bytes), oldest first
    cmd, want = [f"ring {cap}"], []
    wraps = resets = refused = 0
    for _ in range(4000):
        if live and rng.random() < 0.45:
            cmd.append("retire")
            want.append(f"retire {live.pop(0)[0]}")
            continue
        size = 4096 * rng.choice([1, 2, 3, 5, 8, 13, 21, 34, 70])
        cmd.append(f"alloc {size}")
        off = None
        if not live:
            resets += head != 0
            off = 0 if size <= cap else None
        else:
            tail = live[0][0]
            if head > tail:  # free: [head, cap) and [0, tail)
                if head + size <= cap:
                    off = head
                elif size < tail:
                    off, wraps = 0, wraps + 1
            elif head + size < tail:  # wrapped: free is [head, tail)
                off = head
        if off is None:
            refused += 1
            want.append("noroom unchanged")
            continue
        assert all(off + size <= o or o + s <= off for o, s in live) and off + size <= cap
        live.append((off, size))
        head = off + size
        want.append(f"off {off} head {head}")
    assert wraps > 20 and resets > 20 and refused > 20
    same(run(exe, tmp_path, cmd), want)


# ---- 7: the sizes of a batch ------------------------------------------------------------------------------------------
def sizes_as_the_build_states_them(N, n_trees, M, split_after, nstride, hstride, stride8, rows, bits, mb):
    FNODE, LEVELINFO = 48, 32
    max_nodes = M // (split_after + 1) + n_trees
    max_tiles = M // K_TILE + n_trees + max_nodes
    node_of = n_trees * N + 4 if rows else 0
    side_bytes = n_trees * N + 1024 + 16 if rows else 0
    side_bits = (n_trees * N + 31) // 32 + 4 if rows and bits else 0
    arena = max(32 << 20, min(2 * max_nodes * nstride, 16 << 30))
    shadow = max(16 << 20, min(max_nodes * max(hstride, 16), 8 << 30))
    shadow8 = max(16 << 20, min(max_nodes * max(stride8, 16), 4 << 30))
    info_words = (LEVELINFO + (n_trees + 1) * 4 + 3) // 4
    pin_info = (info_words * 4 + 255) & ~255
    pin_nodes = (max_nodes * FNODE + 4095) & ~4095
    pin_head = (3 * pin_info + 256 + 4095) & ~4095
    bounce = min(4096, max(2, mb)) << 20
    return [max_nodes, max_tiles, M, max_nodes, max_tiles, max_tiles * 32, max_tiles, 2 * max_nodes, max_nodes // 256 + 2, node_of,
            side_bytes, side_bits, arena, shadow, shadow8, info_words, pin_info, pin_nodes, pin_head, bounce,
            pin_head + 2 * pin_nodes + bounce]


def test_batch_sizes(exe, tmp_path):
    shapes = [
        (10_000_000, 100, 1_000_000_000, 768, 3200, 1664, 1664, 1, 1, 64),   # 10M x 768 x 100 trees
        (1_000_000, 20, 20_000_000, 1536, 6272, 3200, 3200, 1, 1, 64),        # 1M x 1536 x 20
        (1_000_000, 1, 1_000_000, 768, 3200, 1664, 1664, 0, 0, 64),           # a 1-tree batch
        (10_000_000, 100, 1_000_000_000, 768, 112, 0, 0, 0, 0, 64),           # a 1-bit metric: no shadows, no row-major buffers
        (2_000_000, 8, 16_000_000, 100, 3200, 1664, 0, 1, 0, 64),             # row-major buffers, bytes only
        (2_000_000, 8, 16_000_000, 100, 3200, 1664, 0, 0, 0, 64),             # ... and none
        (500_000, 13, 6_500_000, 768, 3200, 1664, 1664, 1, 1, 1),             # the read-back buffer at its floor
        (500_000, 13, 6_500_000, 768, 3200, 1664, 1664, 1, 0, 100000),        # ... and at its ceiling
        (1_000_000, 6, 123_457, 50, 3200, 0, 0, 0, 0, 64),                    # sub-trees: M != n_trees x N
        (1000, 3, 3000, 2000, 528, 272, 288, 1, 1, 64),                       # nothing splits: the floors of every block
    ]
    cmd = ["sizeof"] + ["sizes " + " ".join(map(str, s)) for s in shapes]
    want = ["sizeof 48 8 8 32 32"] + ["sizes " + " ".join(map(str, sizes_as_the_build_states_them(*s))) for s in shapes]
    same(run(exe, tmp_path, cmd), want)
