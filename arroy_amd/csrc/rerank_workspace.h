// rerank_workspace.h — the device and pinned scratch of one sub-batch of ah_rerank_batch (api.hip: rerank_batch_chunk), written
// down ONCE: a layout is the list of (pointer to carve, elements) in the order the arrays lie in the block, and a Carver walks
// it twice — without a block, to add up the bytes to allocate, then over the block, to hand out the pointers.  Plain C++ with
// no device call, so that tests/rerank_workspace_check.cpp can put the layouts through a sanitizer.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ah {

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// carve arrays (256-byte aligned) out of a linear scratch region; without a region (nullptr) it only counts: every pointer it
// hands out is null and `off` ends as the bytes the same takes need
struct Carver {
    uint8_t *base;
    size_t off = 0;
    explicit Carver(void *b) : base(static_cast<uint8_t *>(b)) {}
    template <typename T>
    T *take(size_t count) {
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += pad256(count * sizeof(T));
        return p;
    }
    // the next `count` elements go to *field; an array the call does not use (`wanted` false) takes nothing and is null
    template <typename T>
    void take(T **field, size_t count, bool wanted = true) {
        *field = wanted ? take<T>(count) : nullptr;
    }
};

struct RerankSizes {  // what the layouts depend on
    size_t nq, dims, row_bytes;  // queries of the sub-batch; the dataset's dimensions and the bytes of one of its rows
    size_t k, total, n_tiles;    // results per query, candidates of all lists, tiles of all lists
    size_t kstride, inv_bytes;   // tournament keys per query; counters of the row-major re-rank (0: not taken)
    size_t hpitch, pitch8;       // halves of a binary16 row, bytes of an int8 row
    bool screened, screened8;    // the certified screen on the binary16 rows / on the int8 rows before that
};

// Bufs: RerankBufs (common.h), or anything with members of those names.  The screen's scratch lies behind everything else.
template <class Bufs>
void rerank_device_layout(Carver &c, const RerankSizes &z, Bufs &b) {
    c.take(&b.d_q_f32, z.nq * z.dims);
    c.take(&b.d_qvecs, z.nq * pad256(z.row_bytes));
    c.take(&b.d_qhdrs, z.nq * 2);
    c.take(&b.d_segs, z.nq);
    c.take(&b.d_tiles, z.n_tiles);
    c.take(&b.d_ids, z.total);
    c.take(&b.d_dist, z.total);
    c.take(&b.d_keys_a, z.nq * z.kstride);
    c.take(&b.d_keys_b, z.nq * z.kstride);
    c.take(&b.d_out_ids, z.nq * z.k);
    c.take(&b.d_out_dist, z.nq * z.k);
    c.take(&b.d_err, 16);  // [error bits][counters of the screened selection]
    c.take(&b.d_inv_counters, z.inv_bytes / 4, z.inv_bytes != 0);
    c.take(&b.d_q16, z.nq * z.hpitch, z.screened);
    c.take(&b.d_qstats, z.nq, z.screened);
    c.take(&b.d_aux, z.total, z.screened);
    c.take(&b.d_q8, z.nq * z.pitch8 * 2, z.screened8);
    c.take(&b.d_q8stats, z.nq, z.screened8);
    c.take(&b.d_aux8, z.total, z.screened8);
}

// the pinned mirrors: what the host writes for the uploads, then what it reads back
template <class Seg, class Tile>
struct RerankPinned {
    float *q, *out_dist;
    Seg *segs;
    Tile *tiles;
    uint32_t *ids, *out_ids, *err;  // err: [error bits][the selection's counters: words 9, 10 of search.hip's SearchStatSlot]
};
template <class Pinned>
void rerank_pinned_layout(Carver &c, const RerankSizes &z, Pinned &p) {
    c.take(&p.q, z.nq * z.dims);
    c.take(&p.segs, z.nq);
    c.take(&p.tiles, z.n_tiles);
    c.take(&p.ids, z.total);
    c.take(&p.out_ids, z.nq * z.k);
    c.take(&p.out_dist, z.nq * z.k);
    c.take(&p.err, 16);
}

}  // namespace ah
