"""Exhausted filters (AH_SEARCH_EXHAUSTED), the part that needs no device.

(a) The fact the feature rests on, on a Python restatement of the reference's loop (src/reader.rs:338-374; the sequential queue
of test_wave_descent_model_cpu.py with ids in the leaves and a candidate set): only KEPT ids count towards search_k, so when
kept_total — the ids the filter keeps summed over every leaf, duplicates across trees included — is at most search_k, the
loop drains its queue and collects exactly K(f), the distinct ids the filter keeps and some leaf holds, whatever the margins
and however equal keys fall.

(b) `plan_exhausted`: the cut of search_batch_cut with the tunable on, in numpy on top of the plans of
test_search_filters_cpu.py / test_search_params_cpu.py.  tests/test_gpu_search_exhausted.py holds the statistics of real calls
against it."""
import ctypes as C
import heapq

import numpy as np

from test_search_filters_cpu import CHUNK_CAP, NO_FILTER
from test_search_params_cpu import BATCH_TOPK_MAX, CHUNK_BYTES, plan as params_plan, query_bytes, stats_of

NEW_SYMBOLS = ("ah_filter_kept_total", "ah_filter_kept_ids", "ah_index_exhausted_stats")


# ---- (a) the model ---------------------------------------------------------------------------------------------------------

class Forest:
    """Random trees over the items 0 .. n_items - 1: node = ("split", left, right, margin) | ("leaf", ids).  Every tree deals
    all items (or, with `holes`, most of them) over its leaves; margins as in test_wave_descent_model_cpu.py: floats, small
    integers, exact zeros, so equal keys are frequent."""

    def __init__(self, rng, n_trees, n_items, depth, tie_level, holes):
        self.nodes, self.roots = [], []
        for _ in range(n_trees):
            ids = rng.permutation(n_items)
            if holes:
                ids = ids[rng.random(n_items) < 0.8]
            self.roots.append(self._grow(rng, ids, depth, tie_level))

    def _grow(self, rng, ids, depth, tie_level):
        if depth == 0 or ids.size <= 2 or rng.random() < 0.15:
            self.nodes.append(("leaf", ids))
            return len(self.nodes) - 1
        cut = int(rng.integers(0, ids.size + 1))  # (an empty side is legal: an empty leaf)
        left = self._grow(rng, ids[:cut], depth - 1, tie_level)
        right = self._grow(rng, ids[cut:], depth - 1, tie_level)
        kind = rng.random()
        if kind < tie_level:
            margin = float(rng.integers(-3, 4))
        elif kind < tie_level + 0.05:
            margin = 0.0
        else:
            margin = float(np.float32(rng.standard_normal() * 2))
        self.nodes.append(("split", left, right, margin))
        return len(self.nodes) - 1


def reference_loop(forest, search_k, candidates):
    """`nns` of Reader::nns_by_leaf before sort + dedup: pop the greatest (key, node id) while fewer than search_k KEPT ids are
    held (reader.rs:341: `while nns.len() < search_k`; :354-360: `descendants & candidates`)."""
    heap = [(-float("inf"), -r) for r in forest.roots]
    heapq.heapify(heap)
    nns = []
    while heap and len(nns) < search_k:
        nk, nn = heapq.heappop(heap)
        key, node = -nk, -nn
        nd = forest.nodes[node]
        if nd[0] == "leaf":
            nns += [int(i) for i in nd[1] if int(i) in candidates]
        else:
            _, left, right, margin = nd
            heapq.heappush(heap, (-min(-margin, key), -left))
            heapq.heappush(heap, (-min(margin, key), -right))
    return nns


def test_a_filter_that_fits_search_k_makes_the_loop_collect_exactly_its_kept_ids():
    rng = np.random.default_rng(20)
    n_exhausted = n_not = 0
    for case in range(3000):
        n_items = int(rng.integers(1, 60))
        f = Forest(rng, int(rng.integers(1, 6)), n_items, int(rng.integers(0, 6)), (0.0, 0.3, 0.9)[case % 3], holes=case % 2 == 1)
        n_cand = int(rng.integers(0, n_items + 1))
        cand = set(rng.choice(n_items + 20, n_cand, replace=False).tolist())  # ids beyond n_items: not stored
        held = np.concatenate([nd[1] for nd in f.nodes if nd[0] == "leaf"] + [np.zeros(0, np.int64)])
        kept_total = int(sum(1 for i in held.tolist() if i in cand))
        kept_ids = sorted(set(held.tolist()) & cand)
        for sk in {kept_total, kept_total + 1, 10 ** 9, max(0, kept_total - 3), max(1, kept_total // 2)}:
            nns = reference_loop(f, sk, cand)
            if kept_total <= sk:  # exhausted: every kept id of every leaf, each once per leaf that holds it
                assert len(nns) == kept_total and sorted(set(nns)) == kept_ids, (case, sk)
                n_exhausted += 1
            else:  # the loop stopped early: nothing is claimed, except that it holds search_k ids and no more than a leaf beyond
                assert len(nns) >= sk and set(nns) <= set(kept_ids), (case, sk)
                n_not += 1
    assert n_exhausted > 3000 and n_not > 1000


# ---- (b) the plan ----------------------------------------------------------------------------------------------------------

def plan_exhausted(slots, kept_totals, sk_effs, counts, group_min, list_lens=None, strides=None, sort=True, row_bytes=0):
    """The cut of one ah_search_batch_filters / _params call with AH_SEARCH_EXHAUSTED=1.

    slots: filter_of_query; kept_totals / list_lens: per filter kept_total(f) and |K(f)| (default: kept_total, one tree);
    sk_effs, counts, strides: per query, or scalars.  Query q is exhausted iff it has a filter and
    kept_total(f) <= sk_eff(q).  The exhausted queries are grouped by slot in the caller's order; those of an empty list are
    answered on the host; the others are cut, effective counts min(count, |K(f)|) within the batched top-k first, into
    sub-batches of one filter that grow while they hold at most 4096 queries and as many times query_bytes(|K(f)|, their
    largest effective count) stay within the chunk budget.  Everything else is cut by the plan of test_search_params_cpu.py.

    Returns {"exhausted": [(slot, query indices, largest effective count)], "empty": indices, "live": indices,
             "rest": [(kind, query indices)]}."""
    slots = np.asarray(slots, dtype=np.uint32)
    nq = slots.size
    sk_effs = np.broadcast_to(np.asarray(sk_effs, dtype=np.int64), (nq,))
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (nq,))
    strides = np.broadcast_to(np.asarray(0 if strides is None else strides, dtype=np.int64), (nq,))
    kept_totals = np.asarray(kept_totals, dtype=np.int64)
    list_lens = kept_totals if list_lens is None else np.asarray(list_lens, dtype=np.int64)
    filtered = slots != NO_FILTER
    gone = np.zeros(nq, dtype=bool)
    gone[filtered] = kept_totals[slots[filtered]] <= sk_effs[filtered]
    exhausted, empty = [], []
    for slot in np.unique(slots[gone]):
        qs = np.flatnonzero(gone & (slots == slot))
        m = int(list_lens[slot])
        if m == 0:
            empty += qs.tolist()
            continue
        eff = np.minimum(counts[qs], m)
        for big in (False, True):
            part = qs[(eff > BATCH_TOPK_MAX) == big]
            c0 = 0
            while c0 < part.size:
                c1, k = c0, 0
                while c1 < part.size and c1 - c0 < CHUNK_CAP:
                    nk = max(k, int(min(counts[part[c1]], m)))
                    if c1 > c0 and (c1 - c0 + 1) * query_bytes(m, nk, row_bytes) > CHUNK_BYTES:
                        break
                    k, c1 = nk, c1 + 1
                exhausted.append((int(slot), part[c0:c1], k))
                c0 = c1
    live = np.flatnonzero(~gone)
    rest = [(kind, live[b]) for kind, b in params_plan(strides[live], counts[live], slots[live], group_min, sort, row_bytes)]
    return {"exhausted": exhausted, "empty": np.asarray(empty, dtype=np.int64), "live": live, "rest": rest}


def stats_of_plan(p, counts, sk_effs, params):
    """(ah_exhausted_stats' call counters, ah_filter_stats', ah_search_stats', ah_params_stats') one call cut as `p` moves."""
    nq = int(p["live"].size + p["empty"].size + sum(b.size for _s, b, _k in p["exhausted"]))
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (nq,))
    sk_effs = np.broadcast_to(np.asarray(sk_effs, dtype=np.int64), (nq,))
    xs = {"queries": nq - int(p["live"].size), "batches": len(p["exhausted"]), "empty_queries": int(p["empty"].size)}
    rest = p["rest"]
    fs = {"calls": 1, "uniform_batches": sum(1 for k, _ in rest if k == "uniform"), "mixed_batches": sum(1 for k, _ in rest if k == "mixed"),
          "uniform_queries": int(sum(b.size for k, b in rest if k == "uniform")), "mixed_queries": int(sum(b.size for k, b in rest if k == "mixed"))}
    ss = {"calls": 1, "queries": int(p["live"].size), "chunks": len(rest)}
    ps = None
    if params:
        ps = stats_of(rest, counts, sk_effs)
        ps["queries"] = nq  # (every query of the call, as ever)
    return xs, fs, ss, ps


def check(p, slots, kept_totals, sk_effs, counts, list_lens):
    slots = np.asarray(slots, dtype=np.uint32)
    nq = slots.size
    sk_effs = np.broadcast_to(np.asarray(sk_effs, dtype=np.int64), (nq,))
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (nq,))
    seen = np.concatenate([b for _s, b, _k in p["exhausted"]] + [p["empty"], p["live"]] + [np.zeros(0, np.int64)])
    assert sorted(seen.tolist()) == list(range(nq)), "every query exactly once"
    assert sorted(np.concatenate([b for _k, b in p["rest"]] + [np.zeros(0, np.int64)]).tolist()) == p["live"].tolist()
    for q in p["live"]:
        assert slots[q] == NO_FILTER or kept_totals[slots[q]] > sk_effs[q]
    for q in p["empty"]:
        assert list_lens[slots[q]] == 0 and kept_totals[slots[q]] <= sk_effs[q]
    for slot, b, k in p["exhausted"]:
        m = int(list_lens[slot])
        assert 0 < b.size <= CHUNK_CAP and m > 0 and (slots[b] == slot).all() and (np.diff(b) > 0).all()
        assert (kept_totals[slot] <= sk_effs[b]).all()
        eff = np.minimum(counts[b], m)
        assert k == eff.max() and ((eff > BATCH_TOPK_MAX).all() or not (eff > BATCH_TOPK_MAX).any())
        assert b.size == 1 or b.size * query_bytes(m, k, 0) <= CHUNK_BYTES


def test_new_symbols_are_exported_and_declared_and_the_tunable_is_off():
    from arroy_amd import _lib
    L = _lib.lib()
    assert L.ah_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert C.sizeof(_lib.AhExhaustedStats) == 6 * 8
    assert _lib.tuning_get("AH_SEARCH_EXHAUSTED")[0] == 0  # off by default: existing statistics of exhausted calls are pinned


def test_refusals_that_need_no_device():
    from arroy_amd import _lib
    L = _lib.lib()
    out = C.c_uint64()
    assert L.ah_filter_kept_total(None, C.byref(out)) == 5 and b"filter is NULL" in L.ah_last_error()
    assert L.ah_filter_kept_ids(None, None, 0, C.byref(out)) == 5 and b"filter is NULL" in L.ah_last_error()
    assert L.ah_index_exhausted_stats(None, None, 0) == 5


def test_plan_the_boundary_and_the_other_kinds():
    # filters: 0 fits (kept_total == sk_eff), 1 does not (one more), 2 keeps nothing that is stored, 3 fits
    kept, lens = np.array([1500, 1512, 0, 12]), np.array([125, 126, 0, 1])
    slots = np.array([0, 1, NO_FILTER, 2, 0, 3, 1, 0, 2, NO_FILTER], dtype=np.uint32)
    p = plan_exhausted(slots, kept, 1500, 25, 16, list_lens=lens)
    check(p, slots, kept, 1500, 25, lens)
    assert [(s, b.tolist(), k) for s, b, k in p["exhausted"]] == [(0, [0, 4, 7], 25), (3, [5], 1)]
    assert p["empty"].tolist() == [3, 8] and p["live"].tolist() == [1, 2, 6, 9]
    assert [(k, b.tolist()) for k, b in p["rest"]] == [("mixed", [2, 9, 1, 6])]
    xs, fs, ss, ps = stats_of_plan(p, 25, 1500, params=False)
    assert xs == {"queries": 6, "batches": 2, "empty_queries": 2} and ss == {"calls": 1, "queries": 4, "chunks": 1}
    assert fs == {"calls": 1, "uniform_batches": 0, "mixed_batches": 1, "uniform_queries": 0, "mixed_queries": 4} and ps is None
    # nothing is exhausted: the plan of ever
    p = plan_exhausted(slots, kept, 10, 25, 16, list_lens=lens)
    assert not p["exhausted"] and p["live"].size == slots.size - 2 and p["empty"].tolist() == [3, 8]  # (kept_total 0 fits any search_k)


def test_plan_per_query_search_k_straddles_and_big_effective_counts_are_apart():
    kept, lens = np.array([25200]), np.array([2100])
    slots = np.zeros(8, dtype=np.uint32)
    sks = np.array([25199, 25200, 30000, 25200, 100, 25200, 25200, 40000])
    counts = np.array([10, 1, 2099, 2100, 5, 2105, 3000, 2048])
    p = plan_exhausted(slots, kept, sks, counts, 16, list_lens=lens)
    check(p, slots, kept, sks, counts, lens)
    # effective counts: 1, 2099, 2100, 2100, 2100, 2048 -> within the batched top-k: queries 1 and 7
    assert [(s, b.tolist(), k) for s, b, k in p["exhausted"]] == [(0, [1, 7], 2048), (0, [2, 3, 5, 6], 2100)]
    assert p["live"].tolist() == [0, 4]


def test_plan_cuts_at_4096_queries_and_at_the_scratch_budget():
    kept, lens = np.array([100]), np.array([100])
    p = plan_exhausted(np.zeros(9000, dtype=np.uint32), kept, 100, 10, 16, list_lens=lens)
    assert [b.size for _s, b, _k in p["exhausted"]] == [4096, 4096, 808]
    big = 200_000  # 1.6 MB of candidates a query: the budget cuts before 4096 queries
    kept, lens = np.array([big]), np.array([big])
    slots = np.zeros(3000, dtype=np.uint32)
    p = plan_exhausted(slots, kept, big, 10, 16, list_lens=lens)
    check(p, slots, kept, big, 10, lens)
    per = CHUNK_BYTES // query_bytes(big, 10, 0)
    assert 1 < per < 3000 and [b.size for _s, b, _k in p["exhausted"]][0] == per


def test_plan_random_calls_keep_the_invariants():
    rng = np.random.default_rng(5)
    for _ in range(300):
        nf = int(rng.integers(1, 9))
        lens = rng.integers(0, 3000, nf)
        kept = lens * int(rng.integers(1, 13))
        nq = int(rng.integers(1, 400))
        slots = rng.integers(0, nf + 1, nq).astype(np.uint32)
        slots[slots == nf] = NO_FILTER
        sks = rng.choice([1, 100, 1500, 10_000, 40_000], nq)
        counts = rng.choice([1, 10, 2048, 2049, 5000], nq)
        p = plan_exhausted(slots, kept, sks, counts, int(rng.choice([1, 16, 1000])), list_lens=lens)
        check(p, slots, kept, sks, counts, lens)
