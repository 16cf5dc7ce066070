// search_call.h — what one call of ah_search_batch / _filters / _params decides from integers before a sub-batch exists: the
// extent of a query (effective search_k, stride of its candidate buffer), the scratch a query costs in a sub-batch, and — for
// the two entry points that cut (search.hip: search_batch_cut) — which queries are answered from their filter's kept list, in
// which sub-batches, and the order and sub-batches of the rest.  The cut is planned in stages, because two facts come from the
// device: kept_total(f) of every referenced filter before plan_split, |K(f)| of every exhausted one before plan_exhausted.
// Plain C++ with no device call, no tunable read and no index or dataset type, so that tests/search_call_check.cpp can run the
// rule on the host, where tests/test_search_call_cpu.py holds it to the numpy restatements of the three search CPU tests.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "search_plan.h"  // kSortLds, kStatusWords, Carver, pad256, AH_NO_FILTER (arroy_hip.h)

namespace ah {

// ---- the top-k kernels' key scratch (batch.hip, distance.hip: both sort kTopkSortKeys keys in LDS) -----------------------------
constexpr uint32_t kTopkSortKeys = 4096;
// the batched tournament top-k takes counts up to half a sort; beyond: the single-query kernels
constexpr bool topk_batch_supported(uint32_t k) { return k <= kTopkSortKeys / 2; }
// keys per query of the tournament over lists of at most max_n candidates
constexpr size_t topk_batch_key_stride(uint32_t max_n) { return (size_t)((max_n + kTopkSortKeys - 1) / kTopkSortKeys) * kTopkSortKeys; }
constexpr uint64_t next_pow2(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
// bytes of the single-query top-k over n keys: a global bitonic sort beyond half a sort, two ping-pong key buffers otherwise
constexpr size_t topk_single_scratch_bytes(uint64_t n, size_t k) {
    return k > kTopkSortKeys / 2 ? (size_t)(next_pow2(n) * 8 + 64)
                                 : (size_t)((n + kTopkSortKeys - 1) / kTopkSortKeys * (uint64_t)kTopkSortKeys * 8 * 2 + 64);
}

// ---- one query ---------------------------------------------------------------------------------------------------------------
// A sub-batch holds at most this many queries, and its scratch (search_query_bytes at its largest stride and count) this much.
constexpr size_t kSearchChunkBytes = 1536ull << 20, kSearchChunkQueries = 4096;

struct IndexExtent {  // what an extent reads of the index; default_oversampling: D::DEFAULT_OVERSAMPLING, 1 or 3 (1-bit rows)
    uint64_t n_trees, desc_len, max_desc;
    uint32_t default_oversampling;
};
struct QueryExtent {
    uint32_t count, sk_eff, stride;
};

// The effective search_k of one query and the capacity of its candidate buffer.  False: search_k too large (a stride of 2^31 - 1
// or more; `out` is then not written) — the callers refuse, naming the query.
inline bool search_extent(const IndexExtent &ix, uint32_t count, uint64_t search_k, uint64_t oversampling, QueryExtent &out) {
    // search_k: reader.rs:330-335; nns can never exceed the blob (every Descendants node is popped at most once)
    unsigned __int128 sk = search_k ? (unsigned __int128)search_k : (unsigned __int128)count * ix.n_trees;
    sk *= oversampling ? oversampling : (uint64_t)ix.default_oversampling;
    const uint64_t sk_eff = (uint64_t)std::min<unsigned __int128>(sk, (unsigned __int128)ix.desc_len);
    uint64_t stride = std::min<uint64_t>(sk_eff + ix.max_desc, ix.desc_len);
    if (stride >= 0x7FFFFFFFull) return false;
    if (stride > kSortLds) stride = std::max<uint64_t>(2, next_pow2(stride));  // the global sort path pads to a power of two
    if (stride >= 0x7FFFFFFFull) return false;
    out = QueryExtent{count, (uint32_t)sk_eff, (uint32_t)stride};
    return true;
}

// Scratch one query of a sub-batch costs at that stride and count.
inline size_t search_query_bytes(size_t row_bytes, uint64_t stride, size_t count) {
    const size_t key_bytes = topk_batch_supported((uint32_t)std::min<size_t>(count, 0xFFFFFFFFu))
                                 ? 2 * topk_batch_key_stride((uint32_t)stride) * 8
                                 : topk_single_scratch_bytes(stride, std::min<size_t>(count, stride)) + 64;
    return (size_t)stride * 8 + key_bytes + count * 8 + row_bytes + 4096;
}

// The fixed sub-batch size of ah_search_batch: nq queries of one extent.
inline size_t search_fixed_chunk(size_t nq, size_t row_bytes, const QueryExtent &e) {
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(nq, kSearchChunkBytes / search_query_bytes(row_bytes, e.stride, e.count)));
    return std::min<size_t>(chunk, kSearchChunkQueries);
}

// ---- a call that is cut ------------------------------------------------------------------------------------------------------
// The queries of one call: an extent each (`per_query`: ah_search_batch_params) or one for all, and a filter slot each.
struct CallQueries {
    size_t nq;
    const QueryExtent *ext;  // nq of them under per_query, else one
    bool per_query;
    const uint32_t *filter_of_query;  // null: slot 0 for all when the call has a filter, none otherwise
    size_t n_filters;
    size_t row_bytes;
    const QueryExtent &ext_of(size_t q) const { return ext[per_query ? q : 0]; }
    uint32_t slot_of(size_t q) const { return filter_of_query ? filter_of_query[q] : (n_filters ? 0u : AH_NO_FILTER); }
};

// The filter slots the queries name, in the order of first reference: kept_total is asked of these, in this order.
inline void referenced_slots(const CallQueries &c, std::vector<uint32_t> &slots) {
    std::vector<uint8_t> known(c.n_filters, 0);
    for (size_t q = 0; q < c.nq; q++) {
        const uint32_t slot = c.slot_of(q);
        if (slot != AH_NO_FILTER && !known[slot]) {
            known[slot] = 1;
            slots.push_back(slot);
        }
    }
}

// Stage A (AH_SEARCH_EXHAUSTED): query q under filter f is exhausted iff kept_total(f) <= its effective search_k.  `gone`: the
// exhausted (slot, query) pairs, ascending = by slot, the caller's order inside; `live`: the other queries in the caller's order.
struct CallSplit {
    std::vector<uint32_t> live;
    std::vector<std::pair<uint32_t, uint32_t>> gone;
    // the slots of `gone`, ascending: the kept list is asked of these, in this order
    void exhausted_slots(std::vector<uint32_t> &slots) const {
        for (size_t g = 0; g < gone.size(); g++)
            if (g == 0 || gone[g].first != gone[g - 1].first) slots.push_back(gone[g].first);
    }
};
inline void plan_split(const CallQueries &c, const uint64_t *kept_total, CallSplit &out) {
    for (size_t q = 0; q < c.nq; q++) {
        const uint32_t slot = c.slot_of(q);
        if (slot != AH_NO_FILTER && kept_total[slot] <= c.ext_of(q).sk_eff) out.gone.push_back({slot, (uint32_t)q});
        else out.live.push_back((uint32_t)q);
    }
    std::sort(out.gone.begin(), out.gone.end());
}

// Stage B: the exhausted queries of one filter, effective counts min(count, |K(f)|) within the batched top-k first, are cut into
// sub-batches that grow while they hold at most kSearchChunkQueries queries and their scratch at stride |K(f)| and their largest
// effective count stays within kSearchChunkBytes; a query whose K(f) is empty is answered by the padding.
struct ExhaustedBatch {
    uint32_t slot, k;  // k: the largest effective count
    size_t a, b;       // queries[a, b) and counts[a, b)
};
struct ExhaustedPlan {
    std::vector<uint32_t> queries, counts;  // the queries of the sub-batches back to back, and the count each asked for
    std::vector<ExhaustedBatch> batches;
    uint64_t n_queries = 0, empty_queries = 0;  // all exhausted queries; those of them with an empty list
};
inline void plan_exhausted(const CallQueries &c, const CallSplit &split, const uint64_t *list_len, ExhaustedPlan &out) {
    const auto &gone = split.gone;
    for (size_t g0 = 0, g1; g0 < gone.size(); g0 = g1) {
        for (g1 = g0 + 1; g1 < gone.size() && gone[g1].first == gone[g0].first;) g1++;
        const uint32_t slot = gone[g0].first, m = (uint32_t)list_len[slot];
        out.n_queries += g1 - g0;
        if (m == 0) out.empty_queries += g1 - g0;
        for (int big = 0; big < 2 && m; big++) {
            std::vector<uint32_t> part;
            for (size_t g = g0; g < g1; g++)
                if ((int)!topk_batch_supported(std::min(c.ext_of(gone[g].second).count, m)) == big) part.push_back(gone[g].second);
            for (size_t c0 = 0, c1; c0 < part.size(); c0 = c1) {
                ExhaustedBatch xb{slot, 0, out.queries.size(), 0};
                for (c1 = c0; c1 < part.size() && c1 - c0 < kSearchChunkQueries; c1++) {
                    const uint32_t kk = std::max(xb.k, std::min(c.ext_of(part[c1]).count, m));
                    if (c1 > c0 && (c1 - c0 + 1) * search_query_bytes(c.row_bytes, m, kk) > kSearchChunkBytes) break;
                    xb.k = kk;
                }
                for (size_t i = c0; i < c1; i++) {
                    out.queries.push_back(part[i]);
                    out.counts.push_back(c.ext_of(part[i]).count);
                }
                xb.b = out.queries.size();
                out.batches.push_back(xb);
            }
        }
    }
}

// Stage C: the order and the sub-batches of the live queries.
//
// The order: stable by filter slot, unfiltered first; inside a slot the queries whose count leaves the batched top-k come last
// and never share a sub-batch with the others; inside such a RUN the queries are ordered stably by the stride of their candidate
// buffer (`sort_by_stride` false: the caller's order).  A run of at least `group_min` queries is cut into UNIFORM sub-batches;
// the queries of the shorter runs are packed, in that order — batched counts, then big ones — into MIXED sub-batches.  A mixed
// sub-batch whose queries happen to share one slot is a uniform one.  Every sub-batch is cut greedily under its OWN largest
// stride and largest count: it grows while it holds at most kSearchChunkQueries queries and its scratch at those maxima stays
// within kSearchChunkBytes.  A sub-batch whose queries do not all share one (count, effective search_k) is VARIED.
struct SubBatch {
    size_t a, b, off;  // perm[a, b); its results are staged from element `off`, in rows of `count`
    bool mixed, varied;
    uint32_t count, sk_eff, stride;  // the largest of its queries
};
struct LivePlan {
    std::vector<uint32_t> perm;  // the live queries in the order of the sub-batches
    std::vector<SubBatch> batches;
    size_t staged = 0;       // elements of all staged rows
    bool any_mixed = false;
    bool identity = true;    // perm[i] == i: the queries are read where the caller put them
    bool direct = true;      // ... and every row is out_stride wide: the results are written where the caller wants them
};
// live: the queries to order (null: all nq of the call, n_live = nq)
inline void plan_live(const CallQueries &c, const uint32_t *live, size_t n_live, size_t group_min, bool sort_by_stride, size_t out_stride,
                      LivePlan &out) {
    auto run_of = [&](size_t q) -> uint64_t {  // (slot, big): the queries of one run share it
        return ((uint64_t)(uint32_t)(c.slot_of(q) + 1u) << 1) | (topk_batch_supported(c.ext_of(q).count) ? 0u : 1u);
    };
    // keys `slot + 1 (mod 2^32)` << 32 | big << 31 | stride, then the query: stable by construction, and no temporary buffer whose
    // allocation std::stable_sort would survive failing — every allocation of a call that fails gives a status
    std::vector<uint32_t> order(n_live);
    {
        std::vector<std::pair<uint64_t, uint32_t>> keyed(n_live);
        for (size_t i = 0; i < n_live; i++) {
            const uint32_t q = live ? live[i] : (uint32_t)i;
            keyed[i] = {(run_of(q) << 31) | (sort_by_stride ? c.ext_of(q).stride : 0u), q};
        }
        std::sort(keyed.begin(), keyed.end());
        for (size_t i = 0; i < n_live; i++) order[i] = keyed[i].second;
    }
    out.perm.reserve(n_live);
    auto cut = [&](const uint32_t *list, size_t n_list, bool may_mix) {
        for (size_t c0 = 0, c1; c0 < n_list; c0 = c1) {
            SubBatch sb{out.perm.size(), 0, out.staged, false, false, 0, 0, 0};
            for (c1 = c0; c1 < n_list && c1 - c0 < kSearchChunkQueries; c1++) {
                const QueryExtent &e = c.ext_of(list[c1]);
                const uint32_t st = std::max(sb.stride, e.stride), cn = std::max(sb.count, e.count);
                if (c1 > c0 && (c1 - c0 + 1) * search_query_bytes(c.row_bytes, st, cn) > kSearchChunkBytes) break;
                sb.stride = st;
                sb.count = cn;
                sb.sk_eff = std::max(sb.sk_eff, e.sk_eff);
            }
            const QueryExtent &first = c.ext_of(list[c0]);
            for (size_t i = c0 + 1; i < c1; i++) {
                sb.mixed = sb.mixed || (may_mix && c.slot_of(list[i]) != c.slot_of(list[c0]));
                sb.varied = sb.varied || c.ext_of(list[i]).count != first.count || c.ext_of(list[i]).sk_eff != first.sk_eff;
            }
            sb.b = sb.a + (c1 - c0);
            out.staged += (c1 - c0) * (size_t)sb.count;
            out.any_mixed = out.any_mixed || sb.mixed;
            out.batches.push_back(sb);
            out.perm.insert(out.perm.end(), list + c0, list + c1);
        }
    };
    std::vector<uint32_t> rest[2];  // the short runs: of batched counts, of big ones
    for (size_t r0 = 0, r1; r0 < n_live; r0 = r1) {
        for (r1 = r0 + 1; r1 < n_live && run_of(order[r1]) == run_of(order[r0]);) r1++;
        if (r1 - r0 >= group_min) cut(order.data() + r0, r1 - r0, false);
        else rest[run_of(order[r0]) & 1u].insert(rest[run_of(order[r0]) & 1u].end(), order.begin() + r0, order.begin() + r1);
    }
    for (const std::vector<uint32_t> &r : rest) cut(r.data(), r.size(), true);
    for (size_t i = 0; i < n_live && out.identity; i++) out.identity = out.perm[i] == i;
    out.direct = out.identity;
    for (const SubBatch &sb : out.batches) out.direct = out.direct && sb.count == out_stride;
}

// ---- the scratch of one exhausted sub-batch (search.hip: search_exhausted) -------------------------------------------------------
// Walked twice by a Carver, as the layouts of search_plan.h are.  Beyond the last array of each lie kExhaustedSlack bytes.
struct ExhaustedSizes {
    size_t nq, dims, row_bytes;  // queries of the sub-batch; the dataset's dimensions and the bytes of one of its rows
    size_t m, k, kstride;        // |K(f)|; the largest effective count; top-k keys per query
};
constexpr size_t kExhaustedSlack = 4096;

// Bufs: ExhaustedBufs (search.hip), or anything with members of those names and element sizes.
template <class Bufs>
void exhausted_device_layout(Carver &c, const ExhaustedSizes &z, Bufs &b) {
    c.take(&b.d_qf32, z.nq * z.dims);
    c.take(&b.d_qrows, z.nq);
    c.take(&b.d_qvecs, z.nq * pad256(z.row_bytes));
    c.take(&b.d_qhdrs, z.nq * 2);
    c.take(&b.d_ids, z.nq * z.m);
    c.take(&b.d_dist, z.nq * z.m);
    c.take(&b.d_segs, z.nq);
    c.take(&b.d_ka, z.nq * z.kstride);
    c.take(&b.d_kb, z.nq * z.kstride);
    c.take(&b.d_oi, z.nq * z.k);
    c.take(&b.d_od, z.nq * z.k);
    c.take(&b.d_err, kStatusWords);
}
template <class Bufs>
void exhausted_pinned_layout(Carver &c, const ExhaustedSizes &z, Bufs &b) {
    c.take(&b.h_q, z.nq * z.dims);
    c.take(&b.h_qrows, z.nq);
    c.take(&b.h_segs, z.nq);
    c.take(&b.h_oi, z.nq * z.k);
    c.take(&b.h_od, z.nq * z.k);
    c.take(&b.h_err, kStatusWords);
}

}  // namespace ah
