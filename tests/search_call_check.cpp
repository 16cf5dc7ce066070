// The call plan of the batched searches (arroy_amd/csrc/search_call.h) on the host, no device: the program reads calls from a
// text file, plans each of them through the stages exactly as search_batch_cut (search.hip) does — the device's two facts,
// kept_total(f) and |K(f)|, come from the file — and prints every plan, with the scratch a query costs at each stated extent (search_query_bytes)
// and, for one extent, the fixed sub-batch size of ah_search_batch (search_fixed_chunk); tests/test_search_call_cpu.py compares the output with
// the numpy restatements of the rule.  It also walks the two scratch layouts of an exhausted sub-batch over a fake block
// (alignment, order, no overlap, the byte totals search_exhausted summed by hand before).  Built with ASan and UBSan.
//
// A call, as whitespace-separated tokens:
//   plan ID MODE n_trees desc_len max_desc default_oversampling row_bytes nq per_query n_filters have_foq exhaust group_min sort out_stride
//   then nq (per_query) or 1 triples — MODE params: count search_k oversampling; MODE extents: count sk_eff stride
//   then, have_foq: nq filter slots; then, exhaust: n_filters kept totals and n_filters list lengths
#include "../arroy_amd/csrc/search_call.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

using namespace ah;

static int failures = 0;
#define CHECK(cond, ...)                             \
    do {                                             \
        if (!(cond)) {                               \
            fprintf(stderr, "FAILED: " __VA_ARGS__); \
            fprintf(stderr, "\n");                   \
            failures++;                              \
        }                                            \
    } while (0)

static void print_list(const char *head, const uint32_t *v, size_t n) {
    fputs(head, stdout);
    for (size_t i = 0; i < n; i++) printf(" %u", v[i]);
    putchar('\n');
}

static bool plan_one(std::ifstream &in) {
    std::string id, mode;
    IndexExtent index{};
    size_t row_bytes, nq, n_filters, group_min, out_stride;
    int per_query, have_foq, exhaust_on, sort;
    if (!(in >> id >> mode >> index.n_trees >> index.desc_len >> index.max_desc >> index.default_oversampling >> row_bytes >> nq >> per_query >>
          n_filters >> have_foq >> exhaust_on >> group_min >> sort >> out_stride))
        return false;
    printf("plan %s\n", id.c_str());
    std::vector<QueryExtent> ext(per_query ? nq : 1);
    long long refused = -1;
    for (size_t q = 0; q < ext.size(); q++) {
        unsigned long long a, b, c;
        if (!(in >> a >> b >> c)) return false;
        if (mode == "extents") ext[q] = QueryExtent{(uint32_t)a, (uint32_t)b, (uint32_t)c};
        else if (!search_extent(index, (uint32_t)a, b, c, ext[q]) && refused < 0) refused = (long long)q;
    }
    std::vector<uint32_t> foq(have_foq ? nq : 0);
    for (uint32_t &s : foq)
        if (!(in >> s)) return false;
    const bool exhaust = exhaust_on && n_filters != 0;  // (the file holds the two tables whenever the tunable is on)
    std::vector<uint64_t> kept_total(exhaust_on ? n_filters : 0), list_len(exhaust_on ? n_filters : 0);
    for (uint64_t &v : kept_total)
        if (!(in >> v)) return false;
    for (uint64_t &v : list_len)
        if (!(in >> v)) return false;
    if (refused >= 0) {
        printf("refused %lld\n", refused);
        return true;
    }
    fputs("extents", stdout);
    for (const QueryExtent &e : ext) printf(" %u %u %u", e.count, e.sk_eff, e.stride);
    putchar('\n');
    fputs("bytes", stdout);  // the scratch each stated extent costs; for one extent, the fixed sub-batch size of ah_search_batch too
    for (const QueryExtent &e : ext) printf(" %zu", search_query_bytes(row_bytes, e.stride, e.count));
    putchar('\n');
    if (!per_query) printf("chunk %zu\n", search_fixed_chunk(nq, row_bytes, ext[0]));
    const CallQueries cq{nq, ext.data(), per_query != 0, have_foq ? foq.data() : nullptr, n_filters, row_bytes};
    CallSplit split;
    ExhaustedPlan xp;
    if (exhaust) {
        std::vector<uint32_t> slots;
        referenced_slots(cq, slots);
        print_list("kept_total_order", slots.data(), slots.size());
        plan_split(cq, kept_total.data(), split);
        slots.clear();
        split.exhausted_slots(slots);
        print_list("kept_list_order", slots.data(), slots.size());
        plan_exhausted(cq, split, list_len.data(), xp);
        for (const ExhaustedBatch &xb : xp.batches) {
            printf("xbatch %u %u :", xb.slot, xb.k);
            for (size_t i = xb.a; i < xb.b; i++) {
                printf(" %u", xp.queries[i]);
                CHECK(xp.counts[i] == cq.ext_of(xp.queries[i]).count, "%s: the count beside an exhausted query is not its own", id.c_str());
            }
            putchar('\n');
        }
        std::vector<uint32_t> empty;
        for (const auto &g : split.gone)
            if (list_len[g.first] == 0) empty.push_back(g.second);
        CHECK(empty.size() == xp.empty_queries && split.gone.size() == xp.n_queries, "%s: the counts of exhausted queries", id.c_str());
        print_list("empty", empty.data(), empty.size());
        print_list("live", split.live.data(), split.live.size());
    }
    LivePlan lp;
    plan_live(cq, exhaust ? split.live.data() : nullptr, exhaust ? split.live.size() : nq, group_min, sort != 0, out_stride, lp);
    for (const SubBatch &sb : lp.batches) {
        printf("sub %s %s %u %u %u %zu :", sb.mixed ? "mixed" : "uniform", sb.varied ? "varied" : "same", sb.count, sb.sk_eff, sb.stride, sb.off);
        for (size_t i = sb.a; i < sb.b; i++) printf(" %u", lp.perm[i]);
        putchar('\n');
    }
    printf("end %zu %d %d %d\n", lp.staged, (int)lp.identity, (int)lp.direct, (int)lp.any_mixed);
    return true;
}

// ---- the scratch of an exhausted sub-batch ----------------------------------------------------------------------------------
struct B16 { uint64_t a, b; };  // RerankSeg
struct Bufs {
    float *d_qf32;
    uint32_t *d_qrows;
    uint8_t *d_qvecs;
    float *d_qhdrs;
    uint32_t *d_ids;
    float *d_dist;
    B16 *d_segs;
    uint64_t *d_ka, *d_kb;
    uint32_t *d_oi;
    float *d_od;
    uint32_t *d_err;
    float *h_q;
    uint32_t *h_qrows;
    B16 *h_segs;
    uint32_t *h_oi;
    float *h_od;
    uint32_t *h_err;
};
struct Arr {
    const char *name;
    const void *p;
    size_t bytes;  // as search_exhausted asks for them
};
// every array lies in the block, 256-aligned, right behind the padded end of the one before it; returns the padded bytes
static size_t walk(const std::vector<Arr> &arrays, const uint8_t *base, size_t block, const ExhaustedSizes &z) {
    size_t sum = 0;
    for (const Arr &a : arrays) {
        const uint8_t *p = static_cast<const uint8_t *>(a.p);
        CHECK(p != nullptr, "nq %zu m %zu k %zu: %s was not handed out", z.nq, z.m, z.k, a.name);
        if (!p) continue;
        CHECK((size_t)(p - base) % 256 == 0, "nq %zu m %zu k %zu: %s is not 256-aligned", z.nq, z.m, z.k, a.name);
        CHECK(p == base + sum, "nq %zu m %zu k %zu: %s is out of order or overlaps", z.nq, z.m, z.k, a.name);
        CHECK(a.bytes > 0 && p + a.bytes <= base + block, "nq %zu m %zu k %zu: %s does not lie inside the block", z.nq, z.m, z.k, a.name);
        sum += pad256(a.bytes);
    }
    return sum;
}
static size_t check_layouts() {
    uint8_t *const dbase = reinterpret_cast<uint8_t *>(uintptr_t(1) << 40), *const pbase = reinterpret_cast<uint8_t *>(uintptr_t(1) << 41);
    size_t n = 0;
    for (size_t nq : {1, 3, 63, 4096})
        for (size_t dims : {1, 32, 768, 1537})
            for (size_t row_bytes : {dims * 4, (dims + 7) / 8 + 8})
                for (size_t m : {1, 125, 4097, 200000})
                    for (size_t k : {1, 25, 2048, 2049, 5000}) {
                        if (k > m) continue;  // an effective count
                        const size_t kstride = topk_batch_supported((uint32_t)k) ? topk_batch_key_stride((uint32_t)m)
                                                                                 : (topk_single_scratch_bytes(m, k) + 15) / 16;
                        const ExhaustedSizes z{nq, dims, row_bytes, m, k, kstride};
                        Bufs count{}, b{};
                        Carver dn(nullptr), pn(nullptr), dv(dbase), pv(pbase);
                        exhausted_device_layout(dn, z, count);
                        exhausted_pinned_layout(pn, z, count);
                        CHECK(!count.d_qf32 && !count.d_err && !count.h_q && !count.h_err, "the counting walk handed out a pointer");
                        exhausted_device_layout(dv, z, b);
                        exhausted_pinned_layout(pv, z, b);
                        CHECK(dv.off == dn.off && pv.off == pn.off, "the two walks of a layout disagree");
                        const size_t qf = nq * dims * 4, words = nq * 4, list = nq * m * 4, keys = nq * kstride * 8, out = nq * k * 4;
                        const size_t dsum = walk({{"d_qf32", b.d_qf32, qf}, {"d_qrows", b.d_qrows, words}, {"d_qvecs", b.d_qvecs, nq * pad256(row_bytes)},
                                                  {"d_qhdrs", b.d_qhdrs, nq * 8}, {"d_ids", b.d_ids, list}, {"d_dist", b.d_dist, list},
                                                  {"d_segs", b.d_segs, nq * 16}, {"d_ka", b.d_ka, keys}, {"d_kb", b.d_kb, keys}, {"d_oi", b.d_oi, out},
                                                  {"d_od", b.d_od, out}, {"d_err", b.d_err, kStatusWords * 4}},
                                                 dbase, dv.off, z);
                        const size_t psum = walk({{"h_q", b.h_q, qf}, {"h_qrows", b.h_qrows, words}, {"h_segs", b.h_segs, nq * 16}, {"h_oi", b.h_oi, out},
                                                  {"h_od", b.h_od, out}, {"h_err", b.h_err, kStatusWords * 4}},
                                                 pbase, pv.off, z);
                        // the totals as search_exhausted summed them by hand
                        CHECK(dn.off + kExhaustedSlack == dsum + 4096, "nq %zu m %zu k %zu: device bytes %zu, summed %zu", nq, m, k, dn.off + kExhaustedSlack, dsum + 4096);
                        CHECK(pn.off + kExhaustedSlack == psum + 4096, "nq %zu m %zu k %zu: pinned bytes %zu, summed %zu", nq, m, k, pn.off + kExhaustedSlack, psum + 4096);
                        n++;
                    }
    return n;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
        return 2;
    }
    static_assert(kSearchChunkQueries == 4096 && kSearchChunkBytes == (1536ull << 20) && kTopkSortKeys == 4096 && kExhaustedSlack == 4096, "the constants");
    const size_t layouts = check_layouts();
    std::ifstream in(argv[1]);
    CHECK(in.good(), "cannot open %s", argv[1]);
    std::string tag;
    size_t n = 0;
    while (in >> tag) {
        if (tag != "plan" || !plan_one(in)) {
            CHECK(false, "call %zu does not parse", n + 1);
            break;
        }
        n++;
    }
    if (failures) return 1;
    printf("done %zu calls %zu layouts\n", n, layouts);
    return 0;
}
