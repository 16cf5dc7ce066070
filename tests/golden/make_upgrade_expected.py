#!/usr/bin/env python3
"""Regenerate tests/golden/upgrade_expected.json and tests/golden/smol_v0_6.mdb from a checkout of the reference:

    python tests/golden/make_upgrade_expected.py /path/to/arroy

Data and expected values only — no reference source code is copied:
  * smol_v0_6.mdb — a byte copy of the test ASSET src/tests/assets/v0_6/smol.mdb (49 152 bytes): one zero normal, one Item
    child, and one node with both.
  * upgrade_expected.json — the two post-upgrade dumps src/tests/upgrade.rs asserts, as parsed records: "smol" from the inline
    snapshot of simple_upgrade_v0_6_to_v0_7, "large" from
    src/tests/snapshots/arroy__tests__upgrade__large_upgrade_v0_6_to_v0_7-10.snap.  Per dump the roots, and per tree node
    {"kind": "split", "left", "right", "normal": true | false} or {"kind": "descendants", "descendants": [...]}.
"""
import json
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def parse_dump(text):
    roots, trees = None, {}
    for line in text.splitlines():
        line = line.strip()
        m = re.match(r"Root: Metadata \{.*roots: \[(.*?)\],", line)
        if m:
            roots = [int(x) for x in m.group(1).split(",") if x.strip()]
            continue
        m = re.match(r"Tree (\d+): Descendants\(Descendants \{ descendants: \[(.*?)\] \}\)", line)
        if m:
            trees[m.group(1)] = {"kind": "descendants", "descendants": [int(x) for x in m.group(2).split(",") if x.strip()]}
            continue
        m = re.match(r"Tree (\d+): SplitPlaneNormal\(SplitPlaneNormal<[\w -]+> \{ left: (\d+), right: (\d+), normal: (.*) \}\)$", line)
        if m:
            normal = m.group(4)
            assert normal == '"none"' or normal.startswith("Leaf {"), normal
            trees[m.group(1)] = {"kind": "split", "left": int(m.group(2)), "right": int(m.group(3)), "normal": normal != '"none"'}
            continue
        assert not line.startswith("Tree "), line
    assert roots is not None and trees
    return {"roots": roots, "trees": trees}


def main(ref):
    shutil.copyfile(os.path.join(ref, "src/tests/assets/v0_6/smol.mdb"), os.path.join(HERE, "smol_v0_6.mdb"))
    src = open(os.path.join(ref, "src/tests/upgrade.rs")).read()
    body = src[src.index("fn simple_upgrade_v0_6_to_v0_7"): src.index("fn large_upgrade_v0_6_to_v0_7")]
    (smol,) = [s for s in re.findall(r'insta::assert_snapshot!\(handle, @r#"(.*?)"#\);', body, re.S) if "Dumping index" in s]
    large = open(os.path.join(ref, "src/tests/snapshots/arroy__tests__upgrade__large_upgrade_v0_6_to_v0_7-10.snap")).read()
    out = {"smol": parse_dump(smol), "large": parse_dump(large)}
    assert len(out["smol"]["trees"]) == 7 and len(out["large"]["trees"]) == 108
    path = os.path.join(HERE, "upgrade_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path, {k: len(v["trees"]) for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
