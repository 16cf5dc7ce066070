"""ah_filter_suspend / ah_filter_resume_batch / ah_index_filters_suspended without a GPU: the symbols against the header and the
ctypes table, the refusals that are judged before a filter is looked at, and the contract of a resume restated in numpy on the
words of the bitmap (`recut`, `apply_edits`, `leaf_counts`: what the kernels do) and checked against plain set arithmetic on every
small case.  tests/test_gpu_filter_resume.py imports the model and holds real calls against it."""
import ctypes as C
import itertools
import os
import re

import numpy as np

from conftest import ROOT

GROUP = 16
NEW_SYMBOLS = ("ah_filter_suspend", "ah_filter_resume_batch", "ah_index_filters_suspended")


def padded_words(len_bits):
    """32-bit words of a filter's bitmap: a multiple of 64 (FilterBlock)."""
    return ((len_bits + 31) // 32 + 63) & ~63


def words_of(ids, len_bits):
    """The padded bitmap words of the ids below len_bits."""
    words = np.zeros(padded_words(len_bits), dtype=np.uint32)
    sel = np.asarray(sorted(ids), dtype=np.int64)
    sel = sel[sel < len_bits]
    np.bitwise_or.at(words, sel >> 5, (np.uint32(1) << (sel & 31).astype(np.uint32)))
    return words


def ids_of(words):
    w = np.asarray(words, dtype=np.uint32)
    return set(np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")).tolist())


def recut(old_words, old_len, new_len):
    """Step 1: the old words below min(old, new) len_bits, the last partial word masked, zero above, padded for new_len."""
    out = np.zeros(padded_words(new_len), dtype=np.uint32)
    keep = min(old_len, new_len)
    whole = keep // 32
    out[:whole] = old_words[:whole]
    if keep % 32:
        out[whole] = old_words[whole] & np.uint32((1 << (keep % 32)) - 1)
    return out


def apply_edits(words, len_bits, remove, add):
    """Step 2: the clears, then the sets; ids at or above len_bits are skipped.  -> (ids_removed, ids_added): the bits each
    launch flipped (an id in both lists that was set is cleared, then set: it counts in both)."""
    flipped = []
    for ids, setting in ((remove, False), (add, True)):
        n = 0
        for i in ids:
            if i >= len_bits:
                continue
            bit = np.uint32(1 << (i & 31))
            was = bool(words[i >> 5] & bit)
            n += was != setting
            words[i >> 5] = (words[i >> 5] | bit) if setting else (words[i >> 5] & ~bit)
        flipped.append(n)
    return tuple(flipped)


def leaf_counts(words, len_bits, kind, offset, count, desc):
    """Step 4: per node slot, the ids of a Descendants node (kind 1) the bitmap holds; 0 for every other slot."""
    out = np.zeros(len(kind), dtype=np.uint32)
    for i in np.flatnonzero((np.asarray(kind) == 1) & (np.asarray(count) > 0)):
        ids = np.asarray(desc[int(offset[i]):int(offset[i]) + int(count[i])], dtype=np.int64)
        ids = ids[ids < len_bits]
        out[i] = int(((words[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).sum())
    return out


def resume_model(old_words, old_len, new_len, remove=(), add=()):
    """-> (the new padded words, listed, ids_removed, ids_added)"""
    words = recut(old_words, old_len, new_len)
    removed, added = apply_edits(words, new_len, sorted(remove), sorted(add))
    return words, int(np.bitwise_count(words).sum()), removed, added


def groups_of(n, group=GROUP):
    return (n + group - 1) // group


def test_new_symbols_are_declared_exported_and_bound():
    from arroy_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "arroy_hip.h")).read()
    declared = set(re.findall(r"^AH_API [^;(]*?\b(ah_[a-z_0-9]+)\s*\(", header, re.M))
    assert "global: ah_*;" in open(os.path.join(ROOT, "arroy_amd", "csrc", "exports.map")).read()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.ah_abi_version() == 7
    assert f"#define AH_FILTER_RESUME_GROUP {GROUP}" in header and _lib.FILTER_RESUME_GROUP == GROUP
    assert _lib.tuning_get("AH_FILTER_RESUME_GROUP") == (GROUP, GROUP)
    assert C.sizeof(_lib.AhFilterEdit) == 4 * C.sizeof(C.c_void_p) and C.sizeof(_lib.AhFilterResumeStats) == 7 * 8
    assert C.sizeof(_lib.AhFilterStats) == 8 * 8  # the layouts existing callers pass have not grown
    assert C.sizeof(_lib.AhSearchStats) == 32 * 8
    assert hasattr(_lib, "FILTER_RESUME_GROUP")


def test_refusals_that_need_no_device():
    from arroy_amd import _lib
    L = _lib.lib()
    st = _lib.AhFilterResumeStats()

    def refused(status, *words):
        assert status == 5, status  # AH_ERR_INVALID_ARGUMENT
        for word in words:
            assert word in L.ah_last_error().decode(), L.ah_last_error()

    refused(L.ah_filter_suspend(None), "filter is NULL")
    out = C.c_uint64(7)
    refused(L.ah_index_filters_suspended(None, C.byref(out)), "NULL argument")
    assert L.ah_filter_resume_batch(None, None, 0, C.byref(st)) == 0 and st.filters == 0  # n == 0: AH_OK, nothing looked at
    refused(L.ah_filter_resume_batch(None, None, 3, C.byref(st)), "filters is NULL")
    three = (C.c_void_p * 3)(None, None, None)
    refused(L.ah_filter_resume_batch(three, None, 3, None), "filters[0] is NULL")
    # the edit lists are judged before any filter: a NULL list with a length, and every place a list can stop ascending
    edits = (_lib.AhFilterEdit * 3)()
    edits[1].n_remove = 2
    refused(L.ah_filter_resume_batch(three, edits, 3, None), "edits[1].remove_sorted is NULL")
    edits[1].n_remove = 0
    edits[2].n_add = 1
    refused(L.ah_filter_resume_batch(three, edits, 3, None), "edits[2].add_sorted is NULL")
    good = np.array([1, 5, 9], np.uint32)
    for bad, pos, what in ((np.array([4, 4, 9], np.uint32), 1, "4 after 4"), (np.array([1, 7, 3], np.uint32), 2, "3 after 7")):
        for field, n_field in (("remove_sorted", "n_remove"), ("add_sorted", "n_add")):
            for i in range(3):
                edits = (_lib.AhFilterEdit * 3)()
                for k in range(3):  # the lists before the bad one are fine
                    edits[k].remove_sorted, edits[k].n_remove = good.ctypes.data, 3
                setattr(edits[i], field, bad.ctypes.data)
                setattr(edits[i], n_field, 3)
                refused(L.ah_filter_resume_batch(three, edits, 3, C.byref(st)), f"edits[{i}].{field} is not strictly ascending",
                        f"position {pos}", what)
    edits = (_lib.AhFilterEdit * 3)()  # all lists empty or ascending: the NULL filter is what is left to refuse
    edits[0].add_sorted, edits[0].n_add = good.ctypes.data, 3
    refused(L.ah_filter_resume_batch(three, edits, 3, None), "filters[0] is NULL")


LENGTHS = (0, 1, 31, 32, 33, 64, 2046, 2047, 2048, 2049)


def test_the_model_equals_set_arithmetic_on_every_small_case():
    """S = ((old - remove) | add) & [0, new_len) for every pair of lengths around a word and around the 2048-bit padding unit,
    with sets that have bits at every edge; the words are those of the list of S, padding included."""
    cases = 0
    for old_len, new_len in itertools.product(LENGTHS, repeat=2):
        edge = {0, 1, 30, 31, 32, 33, 63, 64, 2045, 2046, 2047, 2048}
        universe_old = {i for i in edge if i < old_len}
        olds = [set(), universe_old, {i for i in universe_old if i % 2}, set(range(old_len))]
        for old in olds:
            for remove, add in ((set(), set()), (edge, set()), (set(), edge), ({1, 31, 2047, 5000}, {0, 31, 2046, 2047, 2048, 9999}),
                                (set(range(0, 2100, 3)), set(range(0, 2100, 5)))):
                old_words = words_of(old, old_len)
                words, listed, removed, added = resume_model(old_words, old_len, new_len, remove, add)
                want = {i for i in (old - remove) | add if i < new_len}
                assert ids_of(words) == want, (old_len, new_len, sorted(old)[:5], sorted(remove)[:5], sorted(add)[:5])
                assert np.array_equal(words, words_of(want, new_len)) and words.size == padded_words(new_len)
                assert listed == len(want)
                cut = {i for i in old if i < new_len}
                assert removed == len({i for i in remove if i in cut})
                assert added == len({i for i in add if i < new_len and i not in (cut - remove)})
                cases += 1
    assert cases == len(LENGTHS) ** 2 * 4 * 5
    assert padded_words(0) == 0 and padded_words(1) == 64 and padded_words(2048) == 64 and padded_words(2049) == 128


def test_the_leaf_counts_of_the_model_are_the_intersections():
    rng = np.random.default_rng(3)
    sizes = [0, 1, 7, 8, 9, 63, 64, 65, 300]
    kind, offset, count, desc = [], [], [], []
    for k, c in enumerate(sizes):  # a split node and a free slot between the leaves
        kind += [1, 2, 0]
        offset += [len(desc), 0, 0]
        count += [c, 0, 0]
        desc += rng.choice(3000, c, replace=False).tolist()
    for len_bits in (0, 100, 2048, 3000):
        for held in (set(), set(range(0, 3000, 3)), set(range(3000))):
            words = words_of(held, len_bits)
            got = leaf_counts(words, len_bits, kind, offset, count, np.array(desc + [0]))
            for i in range(len(kind)):
                ids = set(desc[offset[i]:offset[i] + count[i]]) if kind[i] == 1 else set()
                assert got[i] == len({x for x in ids if x in held and x < len_bits}), (len_bits, i)
    assert [groups_of(n) for n in (1, 16, 17, 33)] == [1, 1, 2, 3] and groups_of(33, 1) == 33
