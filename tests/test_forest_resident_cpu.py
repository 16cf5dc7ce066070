"""The host side of a resident forest (arroy_amd/csrc/forest_resident.h: which normal record of which level becomes which
row of the forest's device copy, and where a batch's ids lie in it), checked on the host: a stand-alone program
(tests/forest_resident_check.cpp, its own main, no device call), built once plainly and once with AddressSanitizer and UBSan,
is driven with the node lists of synthetic batches — random trees of counts, their levels laid out as the build lays them out
(by tree; a grouped tail: group after group, each to its end), emitted in post-order — and its printed plan is compared with
the restatement below.  Covered: several batches (rows and ids continue where the batch before stopped), group cuts,
`normal: None` nodes, trees that are a single Descendants root, and node lists that are not the batch's own (refused)."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
from test_index_workspace_cpu import compilers

SRC = os.path.join(ROOT, "tests", "forest_resident_check.cpp")
DESC, SPLIT = 1, 2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("forest_resident_" + request.param) / "forest_resident_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    tried = []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, SRC, "-o", out], capture_output=True, text=True)
        if build.returncode == 0:
            return out
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    raise AssertionError(f"no host compiler built the {request.param} program:\n" + "\n".join(tried))


def run(exe, tmp_path, lines):
    path = tmp_path / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    got = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0 and got.stderr == "", got.stdout[-2000:] + got.stderr[-4000:]
    out = got.stdout.split("\n")
    assert out[-2:] == ["done", ""], out[-3:]
    return out[:-2]


# ---- the model: one batch of trees of counts --------------------------------------------------------------------------------
class Node:
    def __init__(self, tree, start, count, depth):
        self.tree, self.start, self.count, self.depth = tree, start, count, depth
        self.kids = None      # (left, right) of a split node
        self.plane = True     # False: `normal: None`
        self.chunk = self.index = None


def make_batch(rng, tree_counts, split_after, none_share, fork_depth=None, groups=1):
    """Trees of the given item counts, split level by level; the chunks in launch order as (node list); every split node knows its
    chunk and its index inside it.  fork_depth: from that depth on the trees run in `groups` contiguous groups, each to its end."""
    roots, base = [], 0
    for t, cnt in enumerate(tree_counts):
        roots.append(Node(t, base, cnt, 0))
        base += cnt
    chunks = []

    def run_levels(level, depth, stop_at):
        while level and (stop_at is None or depth < stop_at):
            chunk_id = len(chunks)
            chunks.append(level)
            nxt = []
            for i, nd in enumerate(level):  # (ordered by tree, then by parent order)
                nd.chunk, nd.index = chunk_id, i
                nd.plane = rng.random() >= none_share
                left = rng.randint(0, nd.count) if not nd.plane else rng.randint(1, nd.count - 1)
                nd.kids = (Node(nd.tree, nd.start, left, depth + 1), Node(nd.tree, nd.start + left, nd.count - left, depth + 1))
                nxt += [k for k in nd.kids if k.count > split_after]
            level, depth = nxt, depth + 1
        return level, depth

    level, depth = run_levels([r for r in roots if r.count > split_after], 0, fork_depth)
    if level:  # the grouped tail: contiguous ranges of trees, each to its end
        n_trees = len(tree_counts)
        cuts = [n_trees * g // groups for g in range(groups + 1)]
        for g in range(groups):
            run_levels([nd for nd in level if cuts[g] <= nd.tree < cuts[g + 1]], depth, None)
    return roots, chunks, base


def emit(roots, chunk_off, stride, desc_base):
    """The post-order node list (kind, has_normal, offset, count), and the plan it must give: (chunk, index) per plane in order."""
    nodes, planes = [], []

    def walk(nd):
        if nd.kids is None:
            nodes.append((DESC, 0, desc_base + nd.start, nd.count))
            return
        walk(nd.kids[0])
        walk(nd.kids[1])
        nodes.append((SPLIT, 1 if nd.plane else 0, chunk_off[nd.chunk] + nd.index * stride, nd.count))
        if nd.plane:
            planes.append((nd.chunk, nd.index))
    for r in roots:
        walk(r)
    return nodes, planes


def plan_lines(stride, first_row, desc_base, M, chunk_off, chunks, nodes):
    lines = [f"plan {stride} {first_row} {desc_base} {M} {len(chunks)} {len(nodes)}"]
    lines += [f"{chunk_off[c]} {len(chunks[c])}" for c in range(len(chunks))]
    lines += [f"{k} {h} {o} {c}" for k, h, o, c in nodes]
    return lines


def expected(first_row, planes, nodes):
    want = [f"row {c} {i} {first_row + r}" for r, (c, i) in enumerate(planes)]
    held = [(o, o + c) for k, _h, o, c in nodes if k == DESC and c]
    lo, hi = (min(a for a, _ in held), max(b for _, b in held)) if held else (0, 0)
    n_desc = sum(1 for n in nodes if n[0] == DESC)
    n_ids = sum(n[3] for n in nodes if n[0] == DESC)
    n_none = sum(1 for n in nodes if n[0] == SPLIT and not n[1])
    return want + [f"ids {lo} {hi} {n_desc} {n_ids} {n_none}"]


@pytest.mark.parametrize("seed,stride,fork_depth,groups,none_share", [
    (1, 176, None, 1, 0.0),      # level by level, every node with a plane
    (2, 3200, None, 1, 0.15),    # `normal: None` nodes: no row
    (3, 24, 2, 3, 0.1),          # the grouped tail: three groups cut at depth 2 (a BQ stride: 8 + 16 bytes)
    (4, 128, 0, 2, 0.3),         # ... cut at the roots
])
def test_three_batches_continue_rows_and_ids(exe, tmp_path, seed, stride, fork_depth, groups, none_share):
    rng = random.Random(seed)
    split_after = 5
    lines, want = [], []
    first_row, desc_base, normals_base = 0, 0, 0
    for batch in range(3):
        # (a tree of fewer than split_after items is a single Descendants root; one of 0 items holds nothing)
        counts = [rng.choice([0, 3, 5, 6, 40, 97, 150]) for _ in range(rng.randint(2, 5))] + [97]
        roots, chunks, M = make_batch(rng, counts, split_after, none_share, fork_depth, groups)
        chunk_off, at = [], normals_base
        for c in chunks:
            chunk_off.append(at)
            at += len(c) * stride
        nodes, planes = emit(roots, chunk_off, stride, desc_base)
        assert planes and len(chunks) > 1
        lines += plan_lines(stride, first_row, desc_base, M, chunk_off, chunks, nodes)
        want += expected(first_row, planes, nodes)
        first_row += len(planes)
        desc_base += M
        normals_base = at + rng.choice([0, stride, 256])  # (the next batch's levels follow; a gap changes nothing)
    got = run(exe, tmp_path, lines)
    assert got == want


def test_single_node_trees_and_an_empty_batch(exe, tmp_path):
    rng = random.Random(9)
    roots, chunks, M = make_batch(rng, [4, 0, 5], 5, 0.0)
    assert not chunks
    nodes, planes = emit(roots, [], 64, 1000)
    got = run(exe, tmp_path, plan_lines(64, 7, 1000, M, [], chunks, nodes) + ["plan 64 7 0 0 0 0"])
    assert got == ["ids 1000 1009 3 9 0", "ids 0 0 0 0 0"] and not planes


def test_node_lists_that_are_not_the_batchs_own_are_refused(exe, tmp_path):
    rng = random.Random(5)
    stride = 48
    roots, chunks, M = make_batch(rng, [60, 33], 5, 0.0)
    chunk_off, at = [], 480
    for c in chunks:
        chunk_off.append(at)
        at += len(c) * stride
    nodes, planes = emit(roots, chunk_off, stride, 100)
    good = plan_lines(stride, 0, 100, M, chunk_off, chunks, nodes)
    i_split = next(i for i, n in enumerate(nodes) if n[0] == SPLIT)
    i_desc = next(i for i, n in enumerate(nodes) if n[0] == DESC)

    def with_node(i, node, **kw):
        changed = list(nodes)
        changed[i] = node
        return plan_lines(kw.get("stride", stride), kw.get("first_row", 0), 100, M, chunk_off, chunks, changed)
    k, h, o, c = nodes[i_split]
    dk, dh, do, dc = nodes[i_desc]
    cases = [
        with_node(i_split, (k, h, 0, c)),                 # a record below the first chunk
        with_node(i_split, (k, h, o + 4, c)),             # ... between two records
        with_node(i_split, (k, h, at, c)),                # ... behind the last record of the last chunk
        with_node(i_desc, (dk, dh, 99, dc)),              # ids below the batch's range
        with_node(i_desc, (dk, dh, 100 + M, 1)),          # ... behind it
        with_node(i_desc, (0, 0, do, dc)),                # neither kind
        with_node(i_split, (k, h, o, c), first_row=0xFFFFFFFF - len(planes) + 1),  # rows pass 2^32 - 1
        plan_lines(0, 0, 100, M, chunk_off, chunks, nodes),  # no stride
    ]
    lines = list(good)
    for case in cases:
        lines += case
    got = run(exe, tmp_path, lines)
    want = expected(0, planes, nodes)
    assert got[:len(want)] == want and got[len(want):] == ["bad"] * len(cases)
