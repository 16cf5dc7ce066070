"""The inputs of test_gpu_single_topk.py, checked without a GPU: which of the three single-query paths of distance.hip
(k_topk_small, the tournament, the global bitonic sort) each designed list must take, that the lists have the properties they
are named for, and that the two references the GPU answers are compared with — the oracle's restatement of
median_based_top_k and the numpy one of batch_topk_inputs.topk — agree on every new input."""
import numpy as np

import batch_topk_inputs as B
from oracle import oracle as O

agree = B.agree


def test_limits_case_sits_on_both_sides_of_the_one_launch_kernels_limits():
    case = B.limits_case()
    assert [len(r) for r in case.rows] == [n for n, _ in B.LIMITS]
    want = {"1-1": "small", "1023-1023": "small", "1024-1024": "small", "1025-1024": "small", "15361-7": "small",
            "16383-1024": "small", "16384-1024": "small", "5-10": "small",                       # (k = 10 is cut to n = 5)
            "16384-1025": ("tournament", "limits"), "16385-1024": ("tournament", "limits"), "16385-1": ("tournament", "limits")}
    for i, (n, k) in enumerate(B.LIMITS):
        path, why = case.path(i, k)
        name = case.names[i]
        assert (path if path == "small" else (path, why)) == want[name], name
        if path == "small" and n > 1:
            # one span for all lists, scaled bins; with k = 1024 the kernel's 1024 slots are exactly full
            assert why["span"] == 40000 and not why["direct"], name
            assert why["n_sel"] == (B.SEL_CAP if k == B.SEL_CAP else why["n_sel"]) <= B.SEL_CAP, name
    # thread t owns the positions t + 1024 r: 15361 and 1025 leave one item alone in a register slot, 16384 fills the last
    assert 15361 % 1024 == 1 and 1025 % 1024 == 1 and 16384 == 16 * 1024 == B.SMALL_MAX_N
    # a plain random list of 16384 with k = 1024 is served only when the k-th key happens to be the last of its bin (8 keys
    # share a bin); this one is not: the reason for the construction of limits_case
    rng = np.random.default_rng(1)
    d = np.abs(case.c[np.sort(rng.choice(len(case.c), 16384, replace=False))])
    assert B.single_path(d, np.arange(16384), 1024) == ("tournament", "bit3")
    agree(case, sorted({k for _, k in B.LIMITS}))


def test_capacity_case_paths_of_the_one_launch_kernel():
    """`selection` with rule="none": k_topk_small has no sentinel word.  In these lists nothing is skipped anyway (the only
    non-finite words are `wide`'s NaNs, inside the first 2k positions or in a list of n <= 2k), so both rules give one span."""
    case = B.capacity_case(B.CAP_K, B.SINGLE_SPREADS)
    assert len(case) == 5 * len(B.SINGLE_SPREADS)
    for spread in B.SINGLE_SPREADS:
        got = {name: case.path(case.index(f"{spread}-{name}"), B.CAP_K) for name in ("1024", "1025", "k", "bin0", "bin2047")}
        if spread == "wide":   # NaN: declined by bit 2 before any bin is looked at
            assert all(g == ("tournament", "bit2") for g in got.values())
            continue
        assert got["1025"] == ("tournament", "bit3"), spread
        sel = {name: g[1] for name, g in got.items() if name != "1025"}
        assert all(got[name][0] == "small" for name in sel), spread
        assert sel["1024"]["n_sel"] == 1024 and sel["k"]["n_sel"] == B.CAP_K and sel["bin0"]["bin"] == 0, spread
        assert sel["bin2047"]["n_sel"] == B.CAP_K + 10, spread
        for name in sel:  # the same bins with and without the skip
            assert sel[name] == case.select(case.index(f"{spread}-{name}"), B.CAP_K), (spread, name)
        direct = spread in ("consecutive", "span2048")
        assert all(s["direct"] == direct for s in sel.values()), spread
        if not direct:
            assert sel["bin2047"]["bin"] == B.SEL_BINS - 1, spread
    i = case.index("wide-finite-1024")
    w = B.ordered_words(case.dist(i))
    assert int(w.max()) == B.MAX_WORD and int(w.min()) == 0x80000000 and case.path(i, B.CAP_K)[1]["span"] == 2 ** 31 - 2 ** 23
    assert B.MAX_ID not in case.ids.tolist()    # f32::MAX under ordinary ids: never skippable
    # the default arguments still give the batched test's case
    default = B.capacity_case()
    assert default.names == [n for n in case.names if not n.startswith("wide-finite")]
    assert default.c.tobytes() == case.c[: len(default.c)].tobytes()
    agree(case, (B.CAP_K,))


def test_ties_case_at_the_single_query_ks():
    case = B.ties_case()
    for i in range(2):
        for k in B.SINGLE_TIES_K:   # 9000 keys in at most two bins: k_topk_small declines every k it is offered
            assert case.path(i, k) == (("tournament", "bit3") if k <= 1024 else
                                       ("tournament", "limits") if k <= 2048 else ("bitonic", "limits")), (i, k)
            ids, dist = case.expect(i, k)   # equal distances: by position, i.e. ascending ids
            assert np.all((np.diff(dist) > 0) | ((np.diff(dist) == 0) & (np.diff(ids.astype(np.int64)) > 0))), (i, k)
            if i == 0 or k <= 4500:
                assert len(np.unique(dist)) == 1 and ids.tolist() == case.list_ids(i)[case.dist(i) == dist[0]][:k].tolist()
    agree(case, (2049,))


def test_rounds_case_covers_rounds_one_to_five_and_both_buffers_of_the_tournament():
    """launch_topk's tournament has the batched one's shape (chunks of 4096, keep min(k, 2048), round r writes A when r is
    even), so tour_rounds / final_buffer classify its lists too.  k_topk_small takes the short lists at k <= 1024 away from
    it, which is why each list also runs with AH_RERANK_SMALL=0."""
    case = B.rounds_case()
    seen, small = {}, set()
    for i, n in enumerate(B.ROUNDS_N):
        for k in B.ROUNDS_K:
            if n == 0:
                continue
            kk = min(n, k)
            seen[(n, k)] = (B.tour_rounds(n, kk), B.final_buffer(n, kk))
            path, why = case.path(i, k)
            # distinct distances: k_topk_small serves whatever its limits admit, the tournament the rest
            if n <= B.SMALL_MAX_N and kk <= B.SMALL_MAX_K:
                assert path == "small", (n, k, why)
                small.add((n, k))
            else:
                assert (path, why) == ("tournament", "limits"), (n, k)
    assert {r for r, _ in seen.values()} == {1, 2, 3, 4, 5}
    assert {seen[(n, 2048)][0] for n in B.ROUNDS_N if n} == {1, 2, 3, 4, 5}   # k = 2048: a block keeps half its chunk
    for k in B.ROUNDS_K:
        assert {seen[(n, k)][1] for n in B.ROUNDS_N if n} == {"A", "B"}, k
    # AH_RERANK_SMALL=0 is what sends these to a tournament of two rounds (final buffer B)
    assert {(4097, 100), (9000, 1)} <= small and seen[(4097, 100)] == seen[(9000, 1)] == (2, "B")
    # and with the defaults the tournament still sees 1 to 5 rounds and both buffers
    rest = {v for key, v in seen.items() if key not in small}
    assert {r for r, _ in rest} == {1, 2, 3, 4, 5} and {b for _, b in rest} == {"A", "B"}


def test_bitonic_case_pads_to_the_next_power_of_two():
    case = B.bitonic_case()
    assert [len(r) for r in case.rows] == list(B.BITONIC_N)
    pads = []
    for i, n in enumerate(B.BITONIC_N):
        pads.append(1 << (n - 1).bit_length())
        for k in B.bitonic_ks(n):
            assert case.path(i, k) == ("bitonic", "limits"), (n, k)
    assert pads == [4096, 4096, 8192, 16384, 65536]     # one list is a power of two, four need sentinel keys
    assert B.bitonic_ks(40000)[-1] == 40000
    for i, n in enumerate(B.BITONIC_N):
        agree(case, B.bitonic_ks(n), [i])


def test_nonfinite_case_is_decided_by_the_skip_rule_at_every_single_query_k():
    case = B.nonfinite_case(B.SINGLE_NONFINITE_K)
    assert len(case.c) <= 40000 and int(case.ids[-1]) == B.MAX_ID
    default = B.nonfinite_case()    # the default arguments still give the batched test's case, as a prefix
    assert default.names == case.names[: len(default)]
    assert all(default.dist(i).tobytes() == case.dist(i).tobytes() for i in range(len(default)))
    for k in B.SINGLE_NONFINITE_K:
        def differs(name, a, b):
            i = case.index(f"{k}-{name}")
            return case.expect(i, k, a)[0].tolist() != case.expect(i, k, b)[0].tolist()
        assert differs("late-admission", "reference", "every") and differs("max-id-admitted", "reference", "every")
        assert differs("late-admission", "reference", "none") and differs("skip-changes-answer", "reference", "none")
        assert differs("max-id-skipped", "reference", "none")
        assert not differs("mixed", "reference", "none") and not differs("mixed", "reference", "every")
        # the key AT position 2k is skippable and skipped: `pos >= 2k`, not `pos > 2k`
        for name in ("skip-changes-answer", "max-id-skipped"):
            i = case.index(f"{k}-{name}")
            assert B.skipped(case.dist(i), case.list_ids(i), k)[2 * k], (k, name)
        i = case.index(f"{k}-skip-changes-answer")
        got = case.expect(i, k)[1]
        d = case.dist(i).copy()
        d[2 * k] = 0.25    # were that key admitted, it would be the answer's smallest
        assert B.topk(d, case.list_ids(i), k)[1][0] == np.float32(0.25) and got[0] != np.float32(0.25)
        picks = [i for i in range(len(case)) if case.names[i].startswith(f"{k}-")]
        assert len(picks) == 6
        for i in picks:   # k_topk_small declines each (a non-finite distance, or k beyond its limit): the general path answers
            path, why = case.path(i, k)
            assert (path, why) == (("bitonic", "limits") if k > 2048 else ("tournament", "limits" if k > 1024 else "bit2")), case.names[i]
        agree(case, (k,), picks)


def test_by_item_and_all_items_variants_of_the_nonfinite_case():
    case = B.nonfinite_case(B.SINGLE_NONFINITE_K)
    zero = B.with_zero_row(case)
    assert zero.c[0] == 0 and int(zero.ids[0]) == B.ZERO_ID and len(zero.c) == len(case.c) + 1 <= 40000
    od = O.Data(O.MANHATTAN, zero.vectors, ids=zero.ids)
    leaf = od.item_leaf(0)
    for k in B.SINGLE_NONFINITE_K:
        for name in ("late-admission", "mixed", "max-id-admitted"):
            i = zero.index(f"{k}-{name}")
            assert zero.dist(i).tobytes() == case.dist(i).tobytes() and zero.list_ids(i).tolist() == case.list_ids(i).tolist()
            wi, wd = od.rerank(*leaf, zero.rows[i], k)     # by item == by the all-zero query
            ei, ed = case.expect(i, k)
            assert wi.tolist() == ei.tolist() and B.canonical_bits(wd).tolist() == B.canonical_bits(ed).tolist(), (k, name)
        for name in ("max-id-inside", "max-id-skipped", "max-id-admitted"):
            i = case.index(f"{k}-{name}")
            own = B.own_dataset(case, i)
            assert own.dist(0).tobytes() == case.dist(i).tobytes() and int(own.ids[-1]) == B.MAX_ID
            assert not np.array_equal(own.ids, np.arange(len(own.ids)))     # not identity ids: the dataset's id array is read
            agree(own, (k,))
    plain = B.identity_case()
    assert np.array_equal(plain.ids, np.arange(len(plain.ids))) and np.all(np.isfinite(plain.c))
    agree(plain, B.IDENTITY_K)
    assert [plain.path(0, k)[0] for k in B.IDENTITY_K] == ["small", "tournament", "bitonic"]


def test_far_case_puts_skipped_and_counted_keys_in_every_kind_of_block():
    """In the general path every block of the key-making kernel (4096 positions in the tournament's first round, 256 in
    k_make_keys) finds skip_end for itself.  The far lists make the block boundary matter: blocks after the first that want
    skip_end, blocks that skip all their skippable keys because skip_end lies in a later block, the block that holds
    skip_end, blocks after it that skip nothing, and walks of more than one step."""
    for k in B.SINGLE_NONFINITE_K:
        case = B.far_case(k)
        assert case.names == ["far", "far-max-id"] and len(case.c) == 2 * k + B.FAR_RUN + 1 + B.FAR_TAIL + 1 <= 20000
        for i in range(2):
            d, ids = case.dist(i), case.list_ids(i)
            path, why = case.path(i, k)
            assert (path, why) == (("bitonic", "limits") if k > 2048 else ("tournament", "limits" if k > 1024 or len(d) > B.SMALL_MAX_N else "bit2"))
            blocks = B.skip_blocks(d, ids, k, B.KEY_BLOCKS[path])
            first = next(b for b, (wanted, _, _) in enumerate(blocks) if wanted)
            kinds = [what for wanted, what, _ in blocks if wanted]
            assert len(blocks) >= 4 and all(wanted for wanted, _, _ in blocks[first:])           # every block from 2k on walks
            assert kinds.count("all") >= 2 and kinds.count("some") == 1 and kinds.count("none") >= 1
            assert kinds == sorted(kinds, key=["all", "some", "none"].index)
            some = next(b for b, (_, what, _) in enumerate(blocks) if what == "some")
            assert some > first and any(what == "all" and steps > 1 for _, what, steps in blocks)
            assert blocks[some][2] > 4 and all(steps == blocks[some][2] for _, what, steps in blocks if what == "none")
            # skipped keys before skip_end, and keys that count after it, in the block of skip_end and in later blocks
            skipped = B.skipped(d, ids, k)
            skip_end = 2 * k + B.FAR_RUN
            assert skipped[2 * k: skip_end].all() and not skipped[skip_end:].any() and d[skip_end] == np.float32(0.5)
            ei, ed = case.expect(i, k)
            counted = np.flatnonzero(np.isin(ids, ei) & (np.arange(len(d)) > skip_end))
            block = B.KEY_BLOCKS[path]
            assert len(counted) == (5 if i else 4) and len({int(p) // block for p in counted}) >= 2
            assert min(counted) // block == skip_end // block or block == 256
            assert (B.MAX_ID in ei.tolist()) == (i == 1)
            for rule in ("every", "none"):
                assert case.expect(i, k, rule)[0].tolist() != ei.tolist(), (k, i, rule)
        agree(case, (k,))
        own = B.own_dataset(case, 1)
        assert int(own.ids[-1]) == B.MAX_ID and own.dist(0).tobytes() == case.dist(1).tobytes()
        agree(own, (k,))
