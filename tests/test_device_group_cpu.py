"""Device groups without a GPU: the argument checks of ah_group_create and of the group build happen before any device is
touched, and the Python surface without `devices` is the one it always was."""
import ctypes as C
import inspect

import pytest

from arroy_amd import _lib

INVALID = 5


def L():
    return _lib.lib()


def test_group_create_rejects_bad_device_lists_before_any_device_call():
    h = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert L().ah_group_create(2, 8, 10, devs, 0, C.byref(h)) == INVALID  # no device
    assert b"at least one device" in L().ah_last_error()
    assert L().ah_group_create(2, 8, 10, None, 2, C.byref(h)) == INVALID  # NULL list
    assert L().ah_group_create(2, 8, 10, devs, 2, None) == INVALID        # NULL out
    n = _lib.device_count()
    beyond = (C.c_int * 2)(0, n)                                            # index == ah_device_count
    assert L().ah_group_create(2, 8, 10, beyond, 2, C.byref(h)) == INVALID
    assert b"not present" in L().ah_last_error()
    negative = (C.c_int * 1)(-1)
    assert L().ah_group_create(2, 8, 10, negative, 1, C.byref(h)) == INVALID
    assert L().ah_group_create(99, 8, 10, devs, 2, C.byref(h)) == INVALID  # unknown metric
    assert not h.value


def test_group_build_and_handles_reject_null_arguments():
    opt = _lib.AhBuildOptions()
    sink = _lib.NODE_BATCH_FN(lambda _u, _b: 0)
    st = _lib.AhBuildStats()
    assert L().ah_build_forest_group_stream(None, C.byref(opt), sink, None, None, C.byref(st), None) == INVALID
    assert b"group is NULL" in L().ah_last_error()
    out = C.c_void_p()
    assert L().ah_group_member(None, 0, C.byref(out)) == INVALID
    assert L().ah_group_upload_vectors(None, None, None, 0) == INVALID
    assert L().ah_group_upload_records(None, None, None, 0, 0) == INVALID
    assert L().ah_group_finalize(None) == INVALID
    assert L().ah_group_upload_flush(None) == INVALID
    assert L().ah_group_preprocess_dot(None, None) == INVALID
    assert L().ah_group_reserve_build(None, 4, 0) == INVALID
    assert L().ah_group_set_preprocessed(None, 1) == INVALID
    n = C.c_uint32(7)
    assert L().ah_group_size(None, C.byref(n)) == INVALID
    assert L().ah_group_destroy(None) == 0


def test_python_surface_without_devices_is_unchanged():
    import arroy_amd
    from arroy_amd import DatasetGroup
    from arroy_amd.index import ArroyBuilder, Database, Writer
    from arroy_amd import distances as D
    assert "DatasetGroup" in arroy_amd.__all__ and DatasetGroup.member and DatasetGroup.build_stream
    w = Writer(Database(D.Euclidean), 0, 8)
    b = w.builder()
    assert isinstance(b, ArroyBuilder) and b._devices is None and b._group is None
    assert inspect.signature(ArroyBuilder.__init__).parameters["devices"].default is None
    assert inspect.signature(Writer.builder).parameters["devices"].default is None
    with pytest.raises(ValueError):
        w.builder(devices=[])
    # with no items the build touches no device, with or without `devices`
    w.builder(devices=[0, 0]).build()
    w.builder().build()


def _struct_literals(src, name):
    """(line, field names) of every struct-expression `name { ... }` / `name::<..> { ... }` in Rust source `src`."""
    import re
    out = []
    for m in re.finditer(r"\b%s(?:::<[^>{}]*>)?\s*\{" % name, src):
        line_start = src.rfind("\n", 0, m.start()) + 1
        head = src[line_start:m.start()]
        if re.search(r"\b(struct|impl|for|fn)\b", head):  # the definition, an impl header, a signature
            continue
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(src[i], 0)
            i += 1
        body, parts, level, cur = src[m.end():i - 1], [], 0, ""
        for ch in body:
            level += ch in "([{<"
            level -= ch in ")]}>"
            if ch == "," and level == 0:
                parts.append(cur)
                cur = ""
            else:
                cur += ch
        parts.append(cur)
        fields = [re.match(r"\s*(\w+)", p).group(1) for p in parts if p.strip()]
        out.append((src.count("\n", 0, m.start()) + 1, fields))
    return out


def test_every_struct_literal_of_hip_rs_names_every_field():
    """Rust has no default field values: a `HipLeafs { .. }` literal that misses a field added to the struct does not compile.
    Without a Rust toolchain at hand, check every literal of every named-field struct that src/hip.rs defines."""
    import os
    import re

    from conftest import ROOT
    src = open(os.path.join(ROOT, "integration", "arroy-hip", "src", "hip.rs")).read()
    structs = re.findall(r"^pub struct (\w+)(?:<[^>]*>)? \{\n(.*?)^\}", src, re.M | re.S)
    checked = 0
    for name, body in structs:
        fields = re.findall(r"^\s*(?:pub )?(\w+):", body, re.M)
        if not fields or fields == ["_p"]:
            continue
        for line, got in _struct_literals(src, name):
            if any(f.startswith("..") for f in got):
                continue
            assert sorted(got) == sorted(fields), f"hip.rs:{line}: {name} literal has fields {got}, the struct {fields}"
            checked += 1
    assert checked >= 4
