"""integration/arroy-hip: the Rust side of the drop-in as FILES (review item 9).  It cannot be compiled in this image (no
cargo / rustc), but it can be kept applicable and in sync with the C header: the patch must `git apply --check` against
the reference (arroy v0.7.0, pinned line by line by tests/golden/integration_patch_lines.json), be what its generator
produces, and `src/hip.rs` must bind only symbols the header declares, with struct fields in the header's order."""
import hashlib
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

HERE = os.path.join(ROOT, "integration", "arroy-hip")
TOUCHED = {"Cargo.toml", "src/lib.rs", "src/parallel.rs", "src/writer.rs", "src/reader.rs", "src/distance/dot_product.rs"}


def header():
    return open(os.path.join(ROOT, "include", "arroy_hip.h")).read()


def rust():
    return open(os.path.join(HERE, "src", "hip.rs")).read()


def patch_hunks(text):
    """{file: [(first line of the old side, [hunk lines]), ...]} of a unified diff."""
    files, cur = {}, None
    for line in text.splitlines(keepends=True):
        if line.startswith("--- a/"):
            continue
        if line.startswith("+++ b/"):
            cur = files.setdefault(line[6:].rstrip("\n"), [])
            continue
        m = re.match(r"@@ -(\d+)(?:,\d+)? \+\d+(?:,\d+)? @@", line)
        if m:
            cur.append((int(m.group(1)), []))
        else:
            cur[-1][1].append(line)
    return files


def recorded_lines(rel, hunks, edits):
    """{line number: line} of the reference file `rel` as far as the patch (context and removed lines, at their line
    numbers) and the generator's anchors record it.  An anchor goes where it agrees with the most recorded lines, and must
    agree with them everywhere."""
    known = {}
    for start, lines in hunks:
        n = start
        for l in lines:
            if l[0] in " -":
                known[n] = l[1:]
                n += 1
    for before, _after in edits:
        bl = before.splitlines(keepends=True)
        fits = {}
        for o in range(min(known) - len(bl), max(known) + 1):
            got = [known.get(o + i) for i in range(len(bl))]
            if all(g is None or g == t for g, t in zip(got, bl)):
                fits[o] = sum(g is not None for g in got)
        best = max(fits.values(), default=0)
        at = [o for o, v in fits.items() if v == best]
        assert best > 0 and len(at) == 1, f"{rel}: an anchor of make_patch.py does not sit on the patch's lines:\n{before}"
        for i, t in enumerate(bl):
            known[at[0] + i] = t
    return known


def test_patch_applies_to_the_reference_and_matches_its_generator(tmp_path):
    """The six reference files are rebuilt without a checkout of the reference: every line the patch and make_patch.py
    record must be the reference's own line at that number (tests/golden/integration_patch_lines.json: line counts and a
    sha256 per recorded line, made by tests/golden/make_golden.py), every other line is a unique placeholder.  The
    committed patch must apply to them, the generator must run on them (every anchor found once), and the generator's diff
    must produce exactly the files the committed patch produces."""
    patch = os.path.join(HERE, "arroy-hip.patch")
    text = open(patch).read()
    spec = importlib.util.spec_from_file_location("make_patch", os.path.join(HERE, "make_patch.py"))
    make_patch = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make_patch)
    hunks = patch_hunks(text)
    assert set(hunks) == set(make_patch.EDITS) == TOUCHED
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "integration_patch_lines.json")))["files"]
    ref = tmp_path / "reference"
    for rel, hs in hunks.items():
        known = recorded_lines(rel, hs, make_patch.EDITS[rel])
        want = pinned[rel]["sha256"]
        wrong = [n for n in sorted(known) if want.get(str(n)) != hashlib.sha256(known[n].rstrip("\n").encode()).hexdigest()]
        assert not wrong, (f"{rel}: lines {wrong} of arroy-hip.patch / make_patch.py are not the reference's lines at those "
                           "numbers (after a new edit that records new lines: python tests/golden/make_golden.py)")
        assert max(known) <= pinned[rel]["lines"]
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text("".join(known.get(n, f"@@ line {n} @@\n") for n in range(1, pinned[rel]["lines"] + 1)))
    out = subprocess.run([sys.executable, os.path.join(HERE, "make_patch.py"), str(ref)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    (tmp_path / "generated.patch").write_text(out.stdout)
    trees = {}
    for name, p in (("committed", patch), ("generated", str(tmp_path / "generated.patch"))):
        tree = tmp_path / name
        shutil.copytree(ref, tree)
        subprocess.run(["git", "init", "-q", str(tree)], check=True)
        chk = subprocess.run(["git", "apply", "--check", "--verbose", p], cwd=tree, capture_output=True, text=True)
        assert chk.returncode == 0, chk.stderr
        subprocess.run(["git", "apply", p], cwd=tree, check=True)
        trees[name] = {rel: (tree / rel).read_text() for rel in TOUCHED}
    # the files both patches produce, not the patch texts: around the placeholders difflib may align a hunk differently
    # (e.g. where an inserted `}` could pair with either of two) than it does on the whole reference file
    assert trees["committed"] == trees["generated"], \
        "arroy-hip.patch is stale: python integration/arroy-hip/make_patch.py > arroy-hip.patch"
    touched = set(re.findall(r"^\+\+\+ b/(\S+)", text, re.M))
    assert touched == TOUCHED


def test_every_public_function_of_hip_rs_has_a_call_site():
    """Round-5 review: `route_items`, `build_subtrees` and `preprocess_dot` were bindings nothing called — an arroy built with
    `--features hip` still routed every update through rayon.  Every `pub fn` of src/hip.rs must be called from the patch
    (`hip::name(`, `.name(`, `::name(`) or from another function of hip.rs that is."""
    src, patch = rust(), open(os.path.join(HERE, "arroy-hip.patch")).read()
    added = "\n".join(l[1:] for l in patch.splitlines() if l.startswith("+") and not l.startswith("+++"))
    names = re.findall(r"^\s*pub fn (\w+)", src, re.M)
    assert len(names) >= 14, names
    called_from_patch = {n for n in names if re.search(r"(?:hip::|::|\.)%s(?:::<[^>]*>)?\(" % n, added)}
    # transitive closure inside hip.rs: the body of a reachable function names the others it calls
    bodies = {n: src.split("fn %s" % n, 1)[1].split("\n}\n", 1)[0] for n in names}
    reach, grew = set(called_from_patch), True
    while grew:
        grew = False
        for n in list(reach):
            for m in names:
                if m not in reach and re.search(r"\b%s(?:::<[^>]*>)?\(" % m, bodies[n]):
                    reach.add(m)
                    grew = True
    missing = sorted(set(names) - reach)
    assert not missing, f"pub fn of hip.rs without a call site in arroy-hip.patch: {missing}"
    for must in ("route_into_current_trees", "build_large_descendants", "preprocess_dot_records", "search_batch_items", "build_new_trees"):
        assert must in called_from_patch, must


def test_rust_bindings_name_only_declared_symbols():
    declared = set(re.findall(r"^AH_API [^;(]*?\b(ah_[a-z_0-9]+)\s*\(", header(), re.M))
    block = rust().split('extern "C" {', 1)[1].split("\n}\n", 1)[0]
    bound = set(re.findall(r"fn (ah_[a-z_0-9]+)\(", block))
    assert bound and bound <= declared, bound - declared
    assert "AH_ABI_VERSION: c_int = " + re.search(r"#define AH_ABI_VERSION (\d+)", header()).group(1) in rust()


def test_layout_self_checks_are_what_the_header_compiles_to():
    """`const _: () = assert!(size_of::<T>() == ..)` / `offset_of!(T, f) == ..` for every #[repr(C)] struct: the block in
    src/hip.rs must be exactly what tools/gen_layout.py prints from the C compiler's view of include/arroy_hip.h (sizes,
    alignments, offsets: a field whose TYPE drifts no longer compiles on the Rust side)."""
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import gen_layout
    block = gen_layout.block()
    assert block.count("const _: () = assert!(") >= 55
    assert block in rust(), "src/hip.rs: layout block is stale: python integration/arroy-hip/tools/gen_layout.py"
    # every #[repr(C)] struct with fields has its checks
    for name in re.findall(r"#\[repr\(C\)\]\n(?:#\[derive[^\n]*\n)?pub struct (\w+) \{\n    pub (?!_p)", rust()):
        assert f"size_of::<{name}>()" in block, name


@pytest.mark.parametrize("c_name,rust_name", [("ah_build_options", "AhBuildOptions"), ("ah_stream_node", "AhStreamNode"),
                                              ("ah_node_batch", "AhNodeBatch"), ("ah_error_detail", "AhErrorDetail"),
                                              ("ah_node", "AhNode"), ("ah_forest_view", "AhForestView")])
def test_repr_c_structs_follow_the_header(c_name, rust_name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    rs = re.search(r"pub struct %s \{(.*?)\n\}" % rust_name, rust(), re.S).group(1)
    rs_fields = re.findall(r"pub (\w+):", rs)
    # a C declaration `uint32_t left, right;` lists two fields: compare flattened name sequences
    flat = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(",")
        first = re.findall(r"(\w+)\s*$", names[0].replace("*", " "))[0]
        flat.append(first)
        flat += [re.sub(r"[\*\s]", "", x) for x in names[1:]]
    assert rs_fields == flat, (rs_fields, flat)
