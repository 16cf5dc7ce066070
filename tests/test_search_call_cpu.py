"""The call plan of the batched searches (arroy_amd/csrc/search_call.h: the extent of a query, the scratch it costs, which
queries of ah_search_batch_filters / _params are answered from their filter's kept list, and the order and sub-batches of the
rest), run on the host: a stand-alone program (tests/search_call_check.cpp, its own main, no device call) built with
AddressSanitizer and UBSan plans every call of a file written here, and each printed plan is compared with the three numpy
restatements of the rule — test_search_filters_cpu.plan, test_search_params_cpu.extent / query_bytes / plan / stats_of and
test_search_exhausted_cpu.plan_exhausted / stats_of_plan.  No expected value is written down here: all come from those."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_index_workspace_cpu import compilers
from test_search_exhausted_cpu import plan_exhausted, stats_of_plan
from test_search_filters_cpu import CHUNK_CAP, NO_FILTER
from test_search_filters_cpu import plan as filters_plan
from test_search_params_cpu import BATCH_TOPK_MAX, CHUNK_BYTES, SORT_LDS, extent, query_bytes, stats_of
from test_search_params_cpu import plan as params_plan

SRC = os.path.join(ROOT, "tests", "search_call_check.cpp")
INDEX = (10, 5_000_000, 120, 1)  # n_trees, desc_len, max_desc, default oversampling: of the calls that state extents
REFUSED = 0x7FFFFFFF             # a stride from here on is refused ("search_k too large")


class Call:
    """One call as the file states it.  triples: per query (per_query) or one for all — (count, search_k, oversampling) under
    mode "params", (count, effective search_k, stride) under mode "extents".  foq: filter_of_query or None.  kept, lens:
    kept_total(f) and |K(f)| per filter, with AH_SEARCH_EXHAUSTED on (exhaust)."""

    def __init__(self, name, triples, nq=None, per_query=True, mode="extents", index=INDEX, row_bytes=800, n_filters=0, foq=None,
                 exhaust=False, kept=None, lens=None, group_min=16, sort=1, out_stride=None):
        self.name, self.mode, self.index, self.row_bytes, self.per_query = name, mode, index, row_bytes, per_query
        self.triples = [tuple(int(x) for x in t) for t in triples]
        self.nq = len(self.triples) if per_query else int(nq)
        assert len(self.triples) == (self.nq if per_query else 1)
        self.foq = None if foq is None else np.asarray(foq, dtype=np.int64).astype(np.uint32)
        self.n_filters = int(n_filters)
        self.exhaust, self.group_min, self.sort = bool(exhaust), int(group_min), int(sort)
        self.kept = np.asarray(kept if exhaust else [], dtype=np.int64)
        self.lens = np.asarray((kept if lens is None else lens) if exhaust else [], dtype=np.int64)
        assert not exhaust or (self.kept.size == self.lens.size == self.n_filters)
        self.out_stride = max(t[0] for t in self.triples) if out_stride is None else int(out_stride)

    def text(self):
        head = ["plan", self.name, self.mode, *self.index, self.row_bytes, self.nq, int(self.per_query), self.n_filters,
                int(self.foq is not None), int(self.exhaust), self.group_min, self.sort, self.out_stride]
        rows = [" ".join(str(x) for x in head), " ".join(f"{a} {b} {c}" for a, b, c in self.triples)]
        if self.foq is not None:
            rows.append(" ".join(str(int(s)) for s in self.foq))
        if self.exhaust:
            rows += [" ".join(str(int(x)) for x in self.kept), " ".join(str(int(x)) for x in self.lens)]
        return "\n".join(rows) + "\n"

    def extents(self):
        """(counts, effective search_ks, strides) per stated triple by the restatement, or the first refused position."""
        if self.mode == "extents":
            return tuple(np.array(col, dtype=np.int64) for col in zip(*self.triples))
        n_trees, desc_len, max_desc, default = self.index
        got = [extent(c, sk, over, n_trees, desc_len, max_desc, default) for c, sk, over in self.triples]
        for q, (_sk, stride) in enumerate(got):
            if stride >= REFUSED:
                return q
        return (np.array([t[0] for t in self.triples], dtype=np.int64), np.array([g[0] for g in got], dtype=np.int64),
                np.array([g[1] for g in got], dtype=np.int64))

    def slots(self):
        if self.foq is not None:
            return self.foq
        return np.full(self.nq, 0 if self.n_filters else NO_FILTER, dtype=np.uint32)


def parse(text):
    """{name: {"refused": q} | {"extents", "bytes", "chunk", "xbatches", "empty", "live", "subs", "end", "kept_total_order", "kept_list_order"}}"""
    plans, cur = {}, None
    for line in text.splitlines():
        tok = line.split()
        if tok[0] == "plan":
            cur = plans[tok[1]] = {"xbatches": [], "subs": []}
        elif tok[0] == "refused":
            cur["refused"] = int(tok[1])
        elif tok[0] == "extents":
            cur["extents"] = np.array(tok[1:], dtype=np.int64).reshape(-1, 3)
        elif tok[0] in ("kept_total_order", "kept_list_order", "empty", "live", "bytes"):
            cur[tok[0]] = np.array(tok[1:], dtype=np.int64)
        elif tok[0] == "xbatch":
            assert tok[3] == ":"
            cur["xbatches"].append((int(tok[1]), np.array(tok[4:], dtype=np.int64), int(tok[2])))
        elif tok[0] == "sub":
            assert tok[7] == ":" and tok[1] in ("uniform", "mixed") and tok[2] in ("varied", "same")
            cur["subs"].append({"kind": tok[1], "varied": tok[2] == "varied", "count": int(tok[3]), "sk": int(tok[4]), "stride": int(tok[5]),
                                "off": int(tok[6]), "q": np.array(tok[8:], dtype=np.int64)})
        elif tok[0] == "chunk":
            cur["chunk"] = int(tok[1])
        elif tok[0] == "end":
            cur["end"] = tuple(int(x) for x in tok[1:])
        else:
            assert tok[0] == "done", line
    return plans


def compare(call, got):
    """The printed plan of one call against the restatements."""
    name = call.name
    ext = call.extents()
    if isinstance(ext, int):
        assert got == {"xbatches": [], "subs": [], "refused": ext}, name
        return "refused"
    assert "refused" not in got, name
    assert got["extents"].tolist() == np.stack(ext, axis=1).tolist(), name
    nq = call.nq
    # the scratch one query costs at each stated extent, and the fixed sub-batch size of ah_search_batch for one extent
    assert got["bytes"].tolist() == [query_bytes(st, c, call.row_bytes) for c, st in zip(ext[0], ext[2])], name
    if call.per_query:
        assert "chunk" not in got, name
    else:
        assert got["chunk"] == min(CHUNK_CAP, max(1, min(nq, CHUNK_BYTES // query_bytes(ext[2][0], ext[0][0], call.row_bytes)))), name
    counts, sks, strides = (np.broadcast_to(a, (nq,)) for a in ext)
    slots = call.slots()
    if call.exhaust and call.n_filters:
        want = plan_exhausted(slots, call.kept, sks, counts, call.group_min, list_lens=call.lens, strides=strides, sort=call.sort,
                              row_bytes=call.row_bytes)
        named = slots[slots != NO_FILTER]
        _, first = np.unique(named, return_index=True)
        assert got["kept_total_order"].tolist() == named[np.sort(first)].tolist(), name  # the order of first reference
        gone = np.ones(nq, dtype=bool)
        gone[want["live"]] = False
        assert got["kept_list_order"].tolist() == np.unique(slots[gone]).tolist(), name
        assert [(s, b.tolist(), k) for s, b, k in got["xbatches"]] == [(s, b.tolist(), k) for s, b, k in want["exhausted"]], name
        assert got["empty"].tolist() == want["empty"].tolist() and got["live"].tolist() == want["live"].tolist(), name
    else:
        assert not got["xbatches"] and "live" not in got and "kept_total_order" not in got, name
        want = {"exhausted": [], "empty": np.zeros(0, np.int64), "live": np.arange(nq),
                "rest": params_plan(strides, counts, slots, call.group_min, call.sort, call.row_bytes)}
        if not call.per_query:  # one extent for all: the rule ah_search_batch_filters always had, cut where the scratch ends
            per = max(1, min(CHUNK_CAP, CHUNK_BYTES // query_bytes(strides[0], counts[0], call.row_bytes)))
            old = filters_plan(slots, call.group_min, chunk=per)
            assert [(k, b.tolist()) for k, b in old] == [(k, b.tolist()) for k, b in want["rest"]], name
    subs = got["subs"]
    assert [(s["kind"], s["q"].tolist()) for s in subs] == [(k, b.tolist()) for k, b in want["rest"]], name
    off = 0
    for s in subs:  # the largest values of its queries; varied as stats_of says; its rows staged behind the ones before
        b = s["q"]
        assert (s["count"], s["sk"], s["stride"]) == (counts[b].max(), sks[b].max(), strides[b].max()), name
        assert s["varied"] == (np.unique(counts[b]).size > 1 or np.unique(sks[b]).size > 1), name
        assert s["off"] == off, name
        off += b.size * s["count"]
    perm = np.concatenate([s["q"] for s in subs] + [np.zeros(0, np.int64)])
    identity = perm.tolist() == list(range(perm.size))
    direct = identity and all(s["count"] == call.out_stride for s in subs)
    assert got["end"] == (off, int(identity), int(direct), int(any(s["kind"] == "mixed" for s in subs))), name
    # the four stats blocks such a call moves
    n_live = int(want["live"].size)
    xs = {"queries": nq - n_live, "batches": len(got["xbatches"]), "empty_queries": int(got.get("empty", np.zeros(0)).size)}
    fs = {"calls": 1}
    for kind in ("uniform", "mixed"):
        fs[kind + "_batches"] = sum(1 for s in subs if s["kind"] == kind)
        fs[kind + "_queries"] = int(sum(s["q"].size for s in subs if s["kind"] == kind))
    ss = {"calls": 1, "queries": n_live, "chunks": len(subs)}
    ps = {"calls": 1, "batches": len(subs), "varied_batches": sum(1 for s in subs if s["varied"]), "queries": nq,
          "varied_queries": int(sum(s["q"].size for s in subs if s["varied"])),
          "big_count_queries": int(sum(s["q"].size for s in subs if s["count"] > BATCH_TOPK_MAX))}
    wxs, wfs, wss, wps = stats_of_plan(want, counts, sks, params=True)
    assert (xs, fs, ss, ps) == (wxs, wfs, wss, wps), name
    if not call.exhaust:
        assert ps == dict(stats_of(want["rest"], counts, sks), queries=nq), name
    return {"want": want, "subs": subs, "identity": identity, "direct": direct}


def equal(nq, count=25, stride=1700):
    return [(count, stride - 200, stride)] * nq


def cases_of_the_three_modules():
    """The inputs the restatements' own tests use."""
    out = []
    rng = np.random.default_rng(3)
    # test_search_filters_cpu
    for nq in (1, 5, 700):
        for gmin in (1, 16, 1000):
            out.append(Call(f"f_none_{nq}_{gmin}", equal(1), nq=nq, per_query=False, group_min=gmin))
            out.append(Call(f"f_one_{nq}_{gmin}", equal(1), nq=nq, per_query=False, n_filters=1, foq=np.zeros(nq), group_min=gmin))
    for gmin, n in ((2, 100), (1, 100), (5, 1)):
        out.append(Call(f"f_own_{n}_{gmin}", equal(1), nq=n, per_query=False, n_filters=n, foq=np.arange(n), group_min=gmin))
    gmin = 8
    f = np.array([0] * gmin + [1] * (gmin - 1) + [NO_FILTER] * (gmin - 1) + [2] * gmin)
    f = f[rng.permutation(f.size)]
    out.append(Call("f_at_minimum", equal(1), nq=f.size, per_query=False, n_filters=3, foq=f, group_min=gmin))
    out.append(Call("f_at_minimum_one_more", equal(1), nq=f.size + 1, per_query=False, n_filters=3, foq=np.append(f, 1), group_min=gmin))
    rng = np.random.default_rng(4)
    nq = 2 * CHUNK_CAP + 905
    out.append(Call("f_cap_one_run", equal(1), nq=nq, per_query=False, n_filters=1, foq=np.zeros(nq)))
    f = rng.integers(0, 3000, nq)
    out.append(Call("f_cap_short_runs", equal(1), nq=nq, per_query=False, n_filters=3000, foq=f))
    out.append(Call("f_cap_long_run", equal(1), nq=nq, per_query=False, n_filters=3000, foq=np.where(rng.random(nq) < 0.6, 7, f)))
    # test_search_params_cpu
    rng = np.random.default_rng(5)
    for nq in (1, 5, 700, 2 * CHUNK_CAP + 905):
        fs = (np.full(nq, NO_FILTER), np.zeros(nq), rng.integers(0, 9, nq), rng.integers(0, 3000, nq))
        for i, f in enumerate(fs):
            for gmin in ((1, 16, nq + 1) if nq <= 700 else (16,)):
                for count in (25, 5000):
                    for sort in ((0, 1) if nq <= 700 else (1,)):
                        out.append(Call(f"p_equal_{nq}_{i}_{gmin}_{count}_{sort}", equal(nq, count), n_filters=3000, foq=f, group_min=gmin, sort=sort))
    out.append(Call("p_budget_cuts", equal(300, 25, 1 << 20), n_filters=0, foq=np.full(300, NO_FILTER)))
    one_huge = equal(1000)
    one_huge[417] = (25, 1 << 23, 1 << 24)
    for sort in (0, 1):
        out.append(Call(f"p_one_huge_{sort}", one_huge, sort=sort))
    rng = np.random.default_rng(6)
    for gmin in (1, 16, 101):
        for sort in (0, 1):
            counts = np.where(rng.random(100) < 0.4, 2049, 2048)
            stride = rng.choice([300, 1700, 40000], 100)
            out.append(Call(f"p_2048_2049_{gmin}_{sort}", zip(counts, stride - 100, stride), group_min=gmin, sort=sort))
    f = rng.integers(0, 4, 100)
    counts = np.where(rng.random(100) < 0.3, 5000, 10)
    stride = rng.choice([300, 1700, 40000], 100)
    for gmin in (1, 8, 16, 101):
        for sort in (0, 1):
            out.append(Call(f"p_big_under_filters_{gmin}_{sort}", zip(counts, stride - 100, stride), n_filters=4, foq=f, group_min=gmin, sort=sort))
    rng = np.random.default_rng(7)
    for trial in range(40):
        nq = int(rng.integers(1, 900))
        stride = rng.choice([201, 1700, 16300, 32768, 1 << 17, 1 << 20, 1 << 24], nq)
        counts = rng.choice([1, 10, 25, 100, 1024, 1025, 2048, 2049, 5000], nq)
        f = rng.integers(0, int(rng.integers(1, 40)), nq).astype(np.uint32)
        f[rng.random(nq) < 0.2] = NO_FILTER
        for gmin in (1, 16, nq + 1):
            out.append(Call(f"p_random_{trial}_{gmin}_1", zip(counts, stride - 100, stride), n_filters=40, foq=f, group_min=gmin, sort=1,
                            row_bytes=int(rng.integers(4, 7000))))
            out.append(Call(f"p_random_{trial}_{gmin}_0", zip(counts, stride - 100, stride), n_filters=40, foq=f, group_min=gmin, sort=0))
    # test_search_exhausted_cpu
    kept, lens = [1500, 1512, 0, 12], [125, 126, 0, 1]
    slots = [0, 1, NO_FILTER, 2, 0, 3, 1, 0, 2, NO_FILTER]
    for sk in (1500, 10):
        out.append(Call(f"x_boundary_{sk}", [(25, sk, sk + 120)], nq=10, per_query=False, n_filters=4, foq=slots, exhaust=True, kept=kept,
                        lens=lens, row_bytes=0))
    sks = [25199, 25200, 30000, 25200, 100, 25200, 25200, 40000]
    counts = [10, 1, 2099, 2100, 5, 2105, 3000, 2048]
    out.append(Call("x_straddle", zip(counts, sks, np.array(sks) + 120), n_filters=1, foq=np.zeros(8), exhaust=True, kept=[25200], lens=[2100],
                    row_bytes=0))
    out.append(Call("x_4096", [(10, 100, 220)], nq=9000, per_query=False, n_filters=1, foq=np.zeros(9000), exhaust=True, kept=[100], row_bytes=0))
    out.append(Call("x_budget", [(10, 200_000, 1 << 18)], nq=3000, per_query=False, n_filters=1, foq=np.zeros(3000), exhaust=True, kept=[200_000],
                    row_bytes=0))
    rng = np.random.default_rng(5)
    for trial in range(300):
        nf = int(rng.integers(1, 9))
        lens = rng.integers(0, 3000, nf)
        kept = lens * int(rng.integers(1, 13))
        nq = int(rng.integers(1, 400))
        slots = rng.integers(0, nf + 1, nq).astype(np.uint32)
        slots[slots == nf] = NO_FILTER
        sks = rng.choice([1, 100, 1500, 10_000, 40_000], nq)
        counts = rng.choice([1, 10, 2048, 2049, 5000], nq)
        out.append(Call(f"x_random_{trial}", zip(counts, sks, sks + 120), n_filters=nf, foq=slots, exhaust=True, kept=kept, lens=lens,
                        group_min=int(rng.choice([1, 16, 1000])), row_bytes=0))
    return out


def random_calls():
    """Whole calls from (count, search_k, oversampling) on: up to a few thousand queries and 40 filters, with and without
    AH_NO_FILTER, the tunable on and off, both orders."""
    rng = np.random.default_rng(2024)
    out = []
    for trial in range(300):
        index = (int(rng.integers(1, 60)), int(rng.choice([3000, 200_000, 5_000_000, 900_000_000])), int(rng.integers(2, 600)), int(rng.choice([1, 3])))
        nq = int(rng.choice([rng.integers(1, 40), rng.integers(40, 600), rng.integers(600, 5000)], p=[0.3, 0.5, 0.2]))
        nf = int(rng.integers(1, 41))
        counts = rng.choice([1, 10, 25, 100, 1024, 2048, 2049, 5000], nq)
        search_k = rng.choice([0, 0, 50, 1500, 16_000, 17_000, 100_000, 3_000_000], nq)
        over = rng.choice([0, 0, 1, 2, 5], nq)
        slots = rng.integers(0, nf, nq).astype(np.uint32)
        if trial % 2:
            slots[rng.random(nq) < rng.choice([0.1, 0.6])] = NO_FILTER
        if trial % 7 == 0:  # long runs of one slot
            slots[rng.random(nq) < 0.7] = 0
        exhaust = trial % 3 != 0
        lens = rng.choice([0, 1, 30, 1500, 2047, 2048, 2049, 4000, 60_000], nf)
        kept = lens * rng.integers(1, 20, nf)
        sort = int(rng.integers(0, 2))
        if trial % 8 == 5:  # unfiltered, batched counts, the caller's order: one run that stays where it is, its rows unequal
            slots[:], counts, sort = NO_FILTER, np.minimum(counts, 2048), 0
        out.append(Call(f"r_{trial}", zip(counts, search_k, over), mode="params", index=index, n_filters=nf, foq=slots, exhaust=exhaust, kept=kept,
                        lens=lens, group_min=int(rng.choice([1, 4, 16, 64])), sort=sort, row_bytes=int(rng.choice([16, 136, 3072])),
                        out_stride=int(counts.max()) + int(rng.integers(0, 2))))
    return out


def boundary_calls():
    out = []
    # ---- sub-batch size
    for gmin in (1, 8):
        f = [0] * gmin + [1] * max(gmin - 1, 1) + [2] * gmin
        out.append(Call(f"b_group_min_{gmin}", equal(1), nq=len(f), per_query=False, n_filters=3, foq=f, group_min=gmin))
    for nq in (CHUNK_CAP, CHUNK_CAP + 1):
        out.append(Call(f"b_cap_{nq}", equal(1), nq=nq, per_query=False, n_filters=1, group_min=16))
        out.append(Call(f"b_cap_params_{nq}", [(25, 1500 + q % 2, 1700) for q in range(nq)], n_filters=1, group_min=16))
    # ---- byte budget: a power-of-two stride well above the LDS sort; one late query with a larger stride / a larger count
    out.append(Call("b_budget_stride", equal(1, 25, 1 << 20), nq=300, per_query=False))
    late_stride = equal(120, 25, 1 << 19) + equal(1, 25, 1 << 20) + equal(5, 25, 1 << 19)
    out.append(Call("b_budget_late_stride", late_stride, sort=0))
    fit = CHUNK_BYTES // query_bytes(1 << 17, 1, 800)
    out.append(Call("b_budget_late_count", equal(fit - 1, 1, 1 << 17) + equal(1, 2048, 1 << 17) + equal(3, 1, 1 << 17), sort=0))
    # ---- counts and strides: 2048 and 2049 in one slot; 16384 and 16385 (padded to a power of two); sort on and off
    big_index = (10, 900_000_000, 100, 1)
    for sort in (0, 1):
        mixed_counts = [(2049, 0, 0), (2048, 0, 0), (2049, 0, 0), (2048, 30_000, 0), (10, 0, 0)] * 5
        out.append(Call(f"b_2048_2049_{sort}", mixed_counts, mode="params", index=big_index, n_filters=1, group_min=1, sort=sort))
        strides = [(25, SORT_LDS - 100 + d, 0) for d in (1, 0, 1, 0, -1, 1)]
        out.append(Call(f"b_16384_16385_{sort}", strides, mode="params", index=big_index, sort=sort, group_min=1))
    # ---- extent arithmetic
    out.append(Call("b_product_beyond_2_64", [(10, 1 << 63, 4), (10, (1 << 64) - 1, (1 << 32) - 1), (10, 7, 0)], mode="params", index=(10, 3000, 50, 1)))
    huge = (100, (1 << 31) + 5, 64, 1)
    out.append(Call("b_reaches_2_31", [(10, 100, 0), (10, 1 << 40, 0), (10, 1 << 41, 0)], mode="params", index=huge))
    out.append(Call("b_pads_to_2_31", [(10, (1 << 30) - 64, 0), (10, (1 << 30) - 63, 0)], mode="params", index=huge))
    out.append(Call("b_just_below_2_31", [(10, (1 << 30) - 64, 0), (10, (1 << 29) - 32, 2)], mode="params", index=huge))
    out.append(Call("b_default_oversampling_3", [(10, 0, 0), (10, 500, 0), (10, 500, 2)], mode="params", index=(7, 100_000, 40, 3)))
    # ---- exhausted filters
    idx = (10, 5_000_000, 120, 1)
    sk = extent(25, 1500, 0, *idx)[0]
    out.append(Call("b_kept_total_at_sk", [(25, 1500, 0)], nq=6, per_query=False, mode="params", index=idx, n_filters=3, foq=[0, 1, 2, 1, 0, 2],
                    exhaust=True, kept=[sk, sk + 1, 0], lens=[sk // 10, sk // 10, 0]))
    under_one = [(2048, 50_000, 0), (2049, 50_000, 0), (3000, 50_000, 0), (10, 50_000, 0), (2047, 50_000, 0), (10, 100, 0)]
    for m in (2047, 2048, 2049, 2100):
        out.append(Call(f"b_effective_counts_{m}", under_one, mode="params", index=idx, n_filters=1, foq=[0] * 6, exhaust=True, kept=[m * 10], lens=[m]))
    out.append(Call("b_one_filter_no_table", [(25, 1500, 0)], nq=40, per_query=False, mode="params", index=idx, n_filters=1, exhaust=True, kept=[1200],
                    lens=[120]))
    out.append(Call("b_one_filter_no_table_live", [(25, 1500, 0)], nq=40, per_query=False, mode="params", index=idx, n_filters=1, exhaust=True,
                    kept=[1501], lens=[150]))
    out.append(Call("b_no_filters_tunable_on", [(25, 1500, 0)], nq=40, per_query=False, mode="params", index=idx, n_filters=0, exhaust=True, kept=[]))
    # ---- the caller's order kept, rows narrower than out_stride: two sub-batches of unequal widths; one, out_stride beyond it
    out.append(Call("b_callers_order_two_widths", [(10, 0, 0), (25, 400, 0), (2049, 100, 0), (3000, 400, 0)], mode="params", index=idx))
    out.append(Call("b_callers_order_wide_rows", [(10, 100, 0), (25, 400, 0)], mode="params", index=idx, out_stride=36))
    # ---- a mixed tail whose queries happen to share a slot is uniform
    out.append(Call("b_tail_of_one_slot", equal(1), nq=3, per_query=False, n_filters=2, foq=[1, 1, 1], group_min=8))
    out.append(Call("b_tail_after_long_run", equal(1), nq=20, per_query=False, n_filters=2, foq=[0] * 17 + [1] * 3, group_min=8))
    return out


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """Every call of the file, planned by the sanitized program in one run: ({name: Call}, {name: printed plan})."""
    tmp = tmp_path_factory.mktemp("search_call")
    exe, tried = str(tmp / "search_call_check"), []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                SRC, "-o", exe], capture_output=True, text=True)
        if build.returncode == 0:
            break
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    else:
        raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))
    calls = cases_of_the_three_modules() + random_calls() + boundary_calls()
    by_name = {c.name: c for c in calls}
    assert len(by_name) == len(calls)
    path = tmp / "calls.txt"
    path.write_text("".join(c.text() for c in calls))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    last = run.stdout.splitlines()[-1].split()
    assert last[0] == "done" and int(last[1]) == len(calls) and int(last[3]) > 100, last  # ... and the exhausted layouts walked
    plans = parse(run.stdout)
    assert plans.keys() == by_name.keys()
    return by_name, plans


def check(planned, prefix):
    by_name, plans = planned
    seen = {name: compare(call, plans[name]) for name, call in by_name.items() if name.startswith(prefix)}
    assert seen
    return seen


def test_the_inputs_of_the_three_restatements(planned):
    assert len(check(planned, "f_")) > 20 and len(check(planned, "p_")) > 300 and len(check(planned, "x_")) > 300


def test_random_calls(planned):
    seen = check(planned, "r_")
    done = [s for s in seen.values() if s != "refused"]
    assert len(done) >= 250
    # the call shapes search_batch_cut tells apart, each of them many times
    assert sum(1 for s in done if s["identity"] and s["direct"]) > 3 and sum(1 for s in done if not s["identity"]) > 100
    assert sum(1 for s in done if s["identity"] and not s["direct"]) > 3
    assert sum(1 for s in done if s["want"]["exhausted"]) > 50 and sum(1 for s in done if s["want"]["empty"].size) > 20
    assert sum(1 for s in done if any(x["kind"] == "mixed" for x in s["subs"])) > 50


def test_boundaries(planned):
    seen = check(planned, "b_")
    sizes = lambda name: [s["q"].size for s in seen[name]["subs"]]  # noqa: E731
    kinds = lambda name: [s["kind"] for s in seen[name]["subs"]]  # noqa: E731
    # (what follows only states that each call sits where it is meant to: every figure above came from the restatements)
    assert kinds("b_group_min_8") == ["uniform", "uniform", "uniform"] and sizes("b_group_min_8") == [8, 8, 7]
    assert kinds("b_group_min_1") == ["uniform"] * 3
    for kind in ("b_cap_", "b_cap_params_"):
        assert sizes(kind + str(CHUNK_CAP)) == [CHUNK_CAP] and sizes(kind + str(CHUNK_CAP + 1)) == [CHUNK_CAP, 1]
    assert 1 < sizes("b_budget_stride")[0] < 100
    assert sizes("b_budget_late_stride") == [120, 6] and sizes("b_budget_late_count")[1] == 4
    for sort in (0, 1):
        subs = seen[f"b_2048_2049_{sort}"]["subs"]
        assert [s["count"] for s in subs] == [2048, 2049] and not seen[f"b_2048_2049_{sort}"]["identity"]
        assert sorted(set(planned[0][f"b_16384_16385_{sort}"].extents()[2].tolist())) == [SORT_LDS - 1, SORT_LDS, 2 * SORT_LDS]
    assert seen["b_16384_16385_0"]["identity"] and not seen["b_16384_16385_1"]["identity"]
    assert seen["b_reaches_2_31"] == "refused" and seen["b_pads_to_2_31"] == "refused" and seen["b_just_below_2_31"] != "refused"
    x = seen["b_kept_total_at_sk"]["want"]
    assert [b.tolist() for _s, b, _k in x["exhausted"]] == [[0, 4]] and x["empty"].tolist() == [2, 5] and x["live"].tolist() == [1, 3]
    assert [len(seen[f"b_effective_counts_{m}"]["want"]["exhausted"]) for m in (2047, 2048, 2049, 2100)] == [1, 1, 2, 2]
    assert seen["b_one_filter_no_table"]["want"]["live"].size == 0 and seen["b_one_filter_no_table_live"]["want"]["live"].size == 40
    assert kinds("b_no_filters_tunable_on") == ["uniform"] and seen["b_no_filters_tunable_on"]["direct"]
    for name, widths in (("b_callers_order_two_widths", [25, 3000]), ("b_callers_order_wide_rows", [25])):
        assert seen[name]["identity"] and not seen[name]["direct"] and [s["count"] for s in seen[name]["subs"]] == widths
    assert kinds("b_tail_of_one_slot") == ["uniform"] and kinds("b_tail_after_long_run") == ["uniform", "uniform"]
