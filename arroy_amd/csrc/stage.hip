// stage.hip — the host side of getting caller rows into device arrays: ah_dataset_upload_*, ah_group_upload_* and the staging
// pass of an update (update.hip).  Uploads are asynchronous until ah_dataset_finalize: a dataset keeps one Context (stream, ring
// events, device scratch) for all its upload calls; a call returns once its items are COPIED OUT of the caller's pages (the
// contract: no host pointer is used after return) while the last DMA transfers may still be in flight.  The host-side gather
// of a chunk is spread over the worker pool (one core cannot keep a PCIe Gen5 link busy), chunk c+1 is gathered while chunk c
// and c-1 travel.
//
// There is ONE ring loop (stage_loop).  It takes targets — a dataset, or every member of a group — and a source — f32
// vectors or stored records — which says how big an item is, how a slot is laid out, how a chunk is gathered into a slot
// (once, whatever the number of targets) and how a slot is sent to one target on that target's stream.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <immintrin.h>
#include <mutex>
#include <vector>

#include "common.h"

using namespace ah;

namespace {

constexpr int kRing = StageRing::kRing;
constexpr size_t kStageBytes = 32u << 20;  // of one chunk: the rows or records of a ring slot, and their ids

// ---- the id bookkeeping of an append ----------------------------------------------------------------------------------
int check_ids(ah_dataset *ds, const uint32_t *item_ids, size_t n) {
    AH_REQUIRE(!ds->finalized, AH_ERR_INVALID_ARGUMENT, "dataset already finalized");
    AH_REQUIRE(item_ids || n == 0, AH_ERR_INVALID_ARGUMENT, "item_ids is NULL");
    AH_REQUIRE(ds->n + n <= ds->capacity, AH_ERR_INVALID_ARGUMENT, "upload of %zu items exceeds capacity %llu", n,
               (unsigned long long)ds->capacity);
    for (size_t i = 0; i < n; i++) {
        const bool first = ds->n == 0 && i == 0;
        const uint32_t prev = i == 0 ? ds->last_id : item_ids[i - 1];
        AH_REQUIRE(first || item_ids[i] > prev, AH_ERR_INVALID_ARGUMENT,
                   "item ids must be strictly ascending (id %u after %u)", item_ids[i], prev);
    }
    return AH_OK;
}
int check_append(ah_dataset *ds, const uint32_t *item_ids, size_t n) {
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    AH_REQUIRE(!ds->group_member, AH_ERR_INVALID_ARGUMENT, "the dataset is a member of a device group: stage through ah_group_upload_*");
    return check_ids(ds, item_ids, n);
}

// room for n more ids in the host mirror, grown geometrically; called before a group's uploads touch any member, so that
// note_ids (which then allocates nothing) cannot leave one member's ids recorded and another's not
void reserve_ids(ah_dataset *ds, size_t n) {
    const size_t need = ds->h_ids.size() + n;
    if (ds->h_ids.capacity() < need) ds->h_ids.reserve(std::max(need, 2 * ds->h_ids.capacity()));
}

void note_ids(ah_dataset *ds, const uint32_t *item_ids, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if (item_ids[i] != (uint32_t)(ds->n + i)) ds->identity_ids = false;
        ds->h_ids.push_back(item_ids[i]);
    }
    if (n) ds->last_id = item_ids[n - 1];
    ds->n += n;
}

// src/node.rs:252-258: [LEAF_TAG=0][header][vector]; a length mismatch is what UnalignedVector::from_bytes / the dimension
// check reports as InvalidVecDimension
int check_record_len(int metric, uint32_t dims, size_t record_len) {
    const size_t hs = ah_header_size(metric), vs = ah_vector_size(metric, dims);
    if (record_len == 1 + hs + vs) return AH_OK;
    set_error("record length %zu does not match 1 + %zu + %zu for %u dimensions", record_len, hs, vs, dims);
    set_error_status(AH_ERR_INVALID_DIMENSION);
    set_error_detail(0, 1 + hs + vs, record_len);
    return AH_ERR_INVALID_DIMENSION;
}

// ---- the host row copy ---------------------------------------------------------------------------------------------------
// Row copy into the pinned ring with non-temporal stores: the ring is written once and read by the DMA engine, so the
// destination lines need not be read for ownership nor kept in the host caches (a plain memcpy of 3 KB rows moves 3 bytes
// per byte staged; this moves 2).  `dst` is 32-byte aligned (ring rows start on 128-byte lines), `src` is arbitrary —
// LMDB hands out vectors at odd offsets (src/parallel.rs:296-311).
__attribute__((target("avx2"))) void copy_row_stream_avx2(uint8_t *dst, const uint8_t *src, size_t bytes) {
    size_t i = 0;
    for (; i + 128 <= bytes; i += 128) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 32));
        const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 64));
        const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 96));
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), a);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 32), b);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 64), c);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 96), d);
    }
    for (; i + 32 <= bytes; i += 32)
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i)));
    if (i < bytes) memcpy(dst + i, src + i, bytes - i);
}
inline void copy_row(uint8_t *dst, const uint8_t *src, size_t bytes) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2 && !tun(TUN_STAGE_MEMCPY) && bytes >= 512 && (reinterpret_cast<uintptr_t>(dst) & 31u) == 0) copy_row_stream_avx2(dst, src, bytes);
    else memcpy(dst, src, bytes);
}
inline void copy_fence() { _mm_sfence(); }  // non-temporal stores are ordered before the DMA is enqueued

// ---- targets, and the ring a call gathers into ------------------------------------------------------------------------
struct Target {  // where a chunk goes: a dataset, the arrays to write (its own, or the side buffers of an update), its upload context
    ah_dataset *ds;
    StageDst dst;
    Context *ctx;
};
struct Ring {  // kRing pinned slots `stride` bytes apart, however they were obtained, and whose state it is
    uint8_t *base;
    size_t stride;
    StageRing *state;
};

// The dataset's upload context: its stream, its ring events (created lazily) and `scratch` bytes of device scratch, grown
// only once the stream is idle (the old scratch may still be a quantize source).
int upload_context(ah_dataset *ds, size_t scratch, Context **out) {
    AH_HIP(hipSetDevice(ds->device));
    std::lock_guard<std::mutex> lk(ds->up_mu);
    if (!ds->up_ctx) {
        ds->up_ctx = ds->acquire();
        AH_REQUIRE(ds->up_ctx, AH_ERR_DEVICE, "cannot create a HIP stream");
    }
    Context *c = ds->up_ctx;
    for (hipEvent_t &e : c->ev_ring)
        if (!e) AH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (scratch) {
        if (c->d_cap < scratch) AH_HIP(hipStreamSynchronize(c->stream));
        AH_TRY(c->ensure_device(scratch));
    }
    *out = c;
    return AH_OK;
}

// wait until no target's transfer out of ring slot b is in flight
int wait_slot(StageRing &state, const Target *tg, size_t n_tg, int b) {
    if (!state.used[b]) return AH_OK;
    for (size_t i = 0; i < n_tg; i++) AH_HIP(hipEventSynchronize(tg[i].ctx->ev_ring[b]));
    state.used[b] = false;
    return AH_OK;
}

// The ring of a call: kRing slots of at least slot_bytes.  The two rings obtain their memory differently on purpose: a
// dataset's is the pinned scratch of its upload context (Context::ensure_pinned: the NUMA preference, the pinned spare of
// ah_dataset_reserve_build), a group's is one portable block that every member's device reads.  Either is grown only when
// idle: every slot is waited for before the old ring is freed.
int ring_for(const Target *tg, size_t n_tg, ah_group *g, size_t slot_bytes, Ring *out) {
    Context *c0 = tg[0].ctx;
    StageRing &state = g ? g->ring.state : tg[0].ds->up_ring;
    if (g ? g->ring.slot_bytes < slot_bytes : c0->h_cap < (size_t)kRing * slot_bytes) {
        for (int b = 0; b < kRing; b++) AH_TRY(wait_slot(state, tg, n_tg, b));
        if (g) {
            AH_HIP(g->ring.release());
            const size_t slot = (slot_bytes + 4095) & ~(size_t)4095;
            AH_REQUIRE(!fail_alloc_tick(), AH_ERR_OUT_OF_MEMORY, "pinned host allocation of %zu bytes failed (AH_FAIL_ALLOC_AFTER)",
                       slot * kRing);
            AH_HIP(hipHostMalloc(&g->ring.base, slot * kRing, hipHostMallocPortable));
            g->ring.slot_bytes = slot;
        } else {
            AH_TRY(c0->ensure_pinned((size_t)kRing * slot_bytes));
        }
    }
    *out = g ? Ring{reinterpret_cast<uint8_t *>(g->ring.base), g->ring.slot_bytes, &state}
             : Ring{reinterpret_cast<uint8_t *>(c0->h_pinned), c0->h_cap / kRing & ~(size_t)255, &state};
    return AH_OK;
}

// ---- the two sources ---------------------------------------------------------------------------------------------------
// One chunk of an upload in a pinned slot, and the two steps every chunk takes: the gather out of the caller's pages (once,
// whatever the number of targets) and the send to one target on its stream.
struct RecordSlot {  // stored records: rows re-pitched to whole lines, headers and ids apart
    uint8_t *rows, *hdr, *ids;
    RecordSlot(uint8_t *base, size_t chunk, size_t rb, size_t hs)
        : rows(base), hdr(base + pad256(chunk * rb)), ids(base + pad256(chunk * rb) + pad256(chunk * hs)) {}
    static size_t bytes(size_t chunk, size_t rb, size_t hs) { return pad256(chunk * rb) + pad256(chunk * hs) + pad256(chunk * 4); }
};
struct VectorSlot {  // f32 vectors at the staging pitch, then the ids
    float *rows;
    uint8_t *ids;
    VectorSlot(uint8_t *base, size_t chunk, size_t frb) : rows(reinterpret_cast<float *>(base)), ids(base + pad256(chunk * frb)) {}
    static size_t bytes(size_t chunk, size_t frb) { return pad256(chunk * frb) + pad256(chunk * 4); }
};

// LMDB pages -> pinned slot (header and vector split apart, rows re-pitched to 128-byte lines) -> hipMemcpyAsync
struct RecordSource {
    const uint8_t *const *record_ptrs;
    const uint32_t *item_ids;
    size_t rb, hs, vs;  // bytes of a device row, of a header, of a stored vector
    RecordSource(const ah_dataset *ds, const uint8_t *const *ptrs, const uint32_t *ids)
        : record_ptrs(ptrs), item_ids(ids), rb(ds->row_bytes()), hs(ah_header_size(ds->metric)), vs(ah_vector_size(ds->metric, ds->dims)) {}
    size_t item_bytes() const { return rb + hs + 4; }
    size_t slot_bytes(size_t chunk) const { return RecordSlot::bytes(chunk, rb, hs); }
    size_t scratch_bytes(size_t) const { return 0; }
    int gather(uint8_t *base, size_t chunk, size_t done, size_t c) const {
        const RecordSlot slot(base, chunk, rb, hs);
        const uint8_t *const *recs = record_ptrs + done;
        for (size_t i = 0; i < c; i++)
            AH_REQUIRE(recs[i] && recs[i][0] == 0, AH_ERR_INVALID_ARGUMENT, "record %zu is not a leaf (tag %d)", done + i,
                       recs[i] ? recs[i][0] : -1);
        parallel_rows(c, rb + hs, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                memcpy(slot.hdr + i * hs, recs[i] + 1, hs);
                copy_row(slot.rows + i * rb, recs[i] + 1 + hs, vs);
                if (rb > vs) memset(slot.rows + i * rb + vs, 0, rb - vs);
            }
            copy_fence();
        });
        memcpy(slot.ids, item_ids + done, c * 4);
        return AH_OK;
    }
    int send(const Target &t, uint8_t *base, size_t chunk, int, uint64_t row0, size_t c) const {
        const RecordSlot slot(base, chunk, rb, hs);
        hipStream_t s = t.ctx->stream;
        AH_HIP(hipMemcpyAsync(t.dst.rows + row0 * rb, slot.rows, c * rb, hipMemcpyHostToDevice, s));
        AH_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t *>(t.dst.headers) + row0 * hs, slot.hdr, c * hs, hipMemcpyHostToDevice, s));
        AH_HIP(hipMemcpyAsync(t.dst.ids + row0, slot.ids, c * 4, hipMemcpyHostToDevice, s));
        return AH_OK;
    }
};

// Writer::add_item for a batch: f32 rows -> pinned slot -> device, then codec + new_header on the target's device
struct VectorSource {
    const float *vectors;
    const uint32_t *item_ids;
    uint32_t dims;
    bool bq;
    uint32_t fpitch;  // staging pitch in floats
    size_t frb;
    VectorSource(const ah_dataset *ds, const float *v, const uint32_t *ids)
        : vectors(v), item_ids(ids), dims(ds->dims), bq(metric_is_bq(ds->metric)), fpitch(bq ? ((ds->dims + 3u) & ~3u) : ds->pitch),
          frb((size_t)fpitch * 4) {}
    size_t item_bytes() const { return frb + 4; }
    size_t slot_bytes(size_t chunk) const { return VectorSlot::bytes(chunk, frb); }
    // BQ metrics: the f32 rows of slot b land in piece b of the target's device scratch and are quantised from there
    size_t scratch_bytes(size_t chunk) const { return bq ? pad256(chunk * frb) : 0; }
    int gather(uint8_t *base, size_t chunk, size_t done, size_t c) const {
        const VectorSlot slot(base, chunk, frb);
        const float *rows = vectors + done * (size_t)dims;
        parallel_rows(c, frb, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                copy_row(reinterpret_cast<uint8_t *>(slot.rows + i * fpitch), reinterpret_cast<const uint8_t *>(rows + i * (size_t)dims),
                         (size_t)dims * 4);
                for (uint32_t e = dims; e < fpitch; e++) slot.rows[i * fpitch + e] = 0.0f;
            }
            copy_fence();
        });
        memcpy(slot.ids, item_ids + done, c * 4);
        return AH_OK;
    }
    int send(const Target &t, uint8_t *base, size_t chunk, int b, uint64_t row0, size_t c) const {
        const VectorSlot slot(base, chunk, frb);
        const ah_dataset *ds = t.ds;
        hipStream_t s = t.ctx->stream;
        DataView dv = ds->view();  // (the codec and header kernels write into `dst`)
        dv.rows_f32 = bq ? nullptr : reinterpret_cast<const float *>(t.dst.rows);
        dv.rows_bq = bq ? reinterpret_cast<const uint64_t *>(t.dst.rows) : nullptr;
        dv.headers = t.dst.headers;
        if (!bq) {
            AH_HIP(hipMemcpyAsync(t.dst.rows + row0 * frb, slot.rows, c * frb, hipMemcpyHostToDevice, s));
        } else {
            float *d_tmp = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(t.ctx->d_scratch) + (size_t)b * scratch_bytes(chunk));
            AH_HIP(hipMemcpyAsync(d_tmp, slot.rows, c * frb, hipMemcpyHostToDevice, s));
            AH_TRY(launch_quantize_rows(d_tmp, fpitch, ds->dims, reinterpret_cast<uint64_t *>(t.dst.rows) + row0 * ds->pitch, ds->pitch,
                                        ds->words, c, s));
        }
        AH_HIP(hipMemcpyAsync(t.dst.ids + row0, slot.ids, c * 4, hipMemcpyHostToDevice, s));
        AH_TRY(launch_headers_from_vectors(dv, row0, c, s));
        return AH_OK;
    }
};

// ---- the ring loop -------------------------------------------------------------------------------------------------------
struct StageTimes {
    double ctx = 0, gather = 0, wait = 0;  // seconds: contexts + pinned ring, the gathers, waiting for ring slots
};
std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
double secs_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double>(b - a).count();
}

// n items of `src` into rows row0 .. row0 + n of every target's `dst`; `g` is the group whose ring the targets share (nullptr:
// the one target's own).  The caller has checked the ids and keeps the books.
template <class Source>
int stage_loop(Target *tg, size_t n_tg, ah_group *g, const Source &src, uint64_t row0, size_t n, StageTimes *tm) {
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(n, kStageBytes / src.item_bytes()));
    const auto t_begin = now();
    for (size_t i = 0; i < n_tg; i++) AH_TRY(upload_context(tg[i].ds, (size_t)kRing * src.scratch_bytes(chunk), &tg[i].ctx));
    Ring ring;
    AH_TRY(ring_for(tg, n_tg, g, src.slot_bytes(chunk), &ring));
    tm->ctx = secs_between(t_begin, now());
    for (size_t done = 0; done < n;) {
        const size_t c = std::min(chunk, n - done);
        const int b = ring.state->next;
        uint8_t *slot = ring.base + (size_t)b * ring.stride;
        const auto t0 = now();
        AH_TRY(wait_slot(*ring.state, tg, n_tg, b));
        const auto t1 = now();
        AH_TRY(src.gather(slot, chunk, done, c));
        tm->wait += secs_between(t0, t1);
        tm->gather += secs_between(t1, now());
        ring.state->used[b] = true;  // before the sends: one that fails half-way is still waited for
        for (size_t i = 0; i < n_tg; i++) {
            AH_HIP(hipSetDevice(tg[i].ds->device));
            AH_TRY(src.send(tg[i], slot, chunk, b, row0 + done, c));
            AH_HIP(hipEventRecord(tg[i].ctx->ev_ring[b], tg[i].ctx->stream));
        }
        ring.state->next = (b + 1) % kRing;
        done += c;
    }
    return AH_OK;
}

// vectors or records (the one that is not NULL), to either kind of target
int stage_either(Target *tg, size_t n_tg, ah_group *g, const uint32_t *item_ids, const float *vectors,
                 const uint8_t *const *record_ptrs, uint64_t row0, size_t n, StageTimes *tm) {
    return vectors ? stage_loop(tg, n_tg, g, VectorSource(tg[0].ds, vectors, item_ids), row0, n, tm)
                   : stage_loop(tg, n_tg, g, RecordSource(tg[0].ds, record_ptrs, item_ids), row0, n, tm);
}

std::vector<Target> member_targets(ah_group *g) {
    std::vector<Target> tg;
    for (ah_dataset *m : g->members) tg.push_back(Target{m, own_dst(m), nullptr});
    return tg;
}

int upload_flush(ah_dataset *ds) {
    std::lock_guard<std::mutex> lk(ds->up_mu);  // (several threads replicating one unfinalized source flush it together)
    if (!ds->up_ctx) return AH_OK;
    Context *c = ds->up_ctx;
    const hipError_t e = hipStreamSynchronize(c->stream);
    ds->up_ctx = nullptr;
    ds->up_ring = StageRing{};
    ds->release(c);
    if (e != hipSuccess) {
        set_error("staging copy failed: %s", hipGetErrorString(e));
        set_error_status(AH_ERR_DEVICE);
        return AH_ERR_DEVICE;
    }
    return AH_OK;
}

// AH_TIMING=1: where an upload_vectors call's time went (scripts/exp_group.py reads the gather: a group pays it once whatever
// the number of members)
void report_times(size_t n, uint32_t dims, size_t group_members, const StageTimes &tm, double loop_s, double note_s) {
    char to[40] = "";
    if (group_members) snprintf(to, sizeof to, " to %zu members", group_members);
    fprintf(stderr, "[ah] %supload_vectors %zu x %u%s: context + pinned ring %.4f s, gather %.4f s, waiting for the ring %.4f s, "
                    "launch/other %.4f s, note_ids %.4f s\n",
            group_members ? "group " : "", n, dims, to, tm.ctx, tm.gather, tm.wait, loop_s - tm.ctx - tm.gather - tm.wait, note_s);
}

// the body of a group upload: the chunk is gathered once into the group's pinned ring and sent from that same slot to every
// member, each on its own stream, where the codec / header kernels run on the member's device
int group_upload(ah_group *g, const uint32_t *item_ids, const float *vectors, const uint8_t *const *record_ptrs, size_t n) {
    DeviceRestore restore_device;
    for (ah_dataset *m : g->members) reserve_ids(m, n);
    const auto t_begin = now();
    StageTimes tm;
    std::vector<Target> tg = member_targets(g);
    AH_TRY(stage_either(tg.data(), tg.size(), g, item_ids, vectors, record_ptrs, g->members[0]->n, n, &tm));
    const auto t_loop = now();
    for (ah_dataset *m : g->members) note_ids(m, item_ids, n);
    if (vectors && tun(TUN_TIMING) != 0)
        report_times(n, g->dims, g->members.size(), tm, secs_between(t_begin, t_loop), secs_between(t_loop, now()));
    return AH_OK;
}

}  // namespace

namespace ah {
int flush_staging(ah_dataset *ds) { return upload_flush(ds); }

int flush_staging(ah_group *g) {
    int st = AH_OK;
    for (ah_dataset *m : g->members) {
        const int s = upload_flush(m);
        if (st == AH_OK) st = s;
    }
    g->ring.state = StageRing{};
    return st;
}

int stage_items(const std::vector<ah_dataset *> &members, ah_group *g, const StageDst *dst, const uint32_t *item_ids,
                const float *vectors, const uint8_t *const *record_ptrs, size_t n) {
    std::vector<Target> tg;
    for (size_t i = 0; i < members.size(); i++) tg.push_back(Target{members[i], dst[i], nullptr});
    StageTimes tm;
    const int st = stage_either(tg.data(), tg.size(), g, item_ids, vectors, record_ptrs, 0, n, &tm);
    const int fl = g ? flush_staging(g) : flush_staging(members[0]);  // (after a failure too: nothing stays in flight)
    return st != AH_OK ? st : fl;
}
}  // namespace ah

extern "C" {

int ah_dataset_upload_records(ah_dataset *ds, const uint32_t *item_ids, const uint8_t *const *record_ptrs,
                              size_t record_len, size_t n) {
    AH_GUARDED("ah_dataset_upload_records")
    AH_TRY(check_append(ds, item_ids, n));
    if (n == 0) return AH_OK;
    AH_REQUIRE(item_ids && record_ptrs, AH_ERR_INVALID_ARGUMENT, "NULL input");
    AH_TRY(check_record_len(ds->metric, ds->dims, record_len));
    Target t{ds, own_dst(ds), nullptr};
    StageTimes tm;
    AH_TRY(stage_loop(&t, 1, nullptr, RecordSource(ds, record_ptrs, item_ids), ds->n, n, &tm));
    note_ids(ds, item_ids, n);
    // The stored DotProduct headers are taken as they are: items written by `Writer::add_item` carry {0, 0} until
    // `DotProduct::preprocess` ran over the database (src/distance/dot_product.rs:119-165), so the dataset still needs
    // ah_preprocess_dot unless the caller states that the database was preprocessed (ah_dataset_set_preprocessed).
    return AH_OK;
    AH_GUARDED_END
}

int ah_dataset_upload_vectors(ah_dataset *ds, const uint32_t *item_ids, const float *vectors, size_t n) {
    AH_GUARDED("ah_dataset_upload_vectors")
    AH_TRY(check_append(ds, item_ids, n));
    if (n == 0) return AH_OK;
    AH_REQUIRE(item_ids && vectors, AH_ERR_INVALID_ARGUMENT, "NULL input");
    Target t{ds, own_dst(ds), nullptr};
    const VectorSource src(ds, vectors, item_ids);
    // Rows that need no re-pitching can travel straight from the caller's memory when it is (or can be) page-locked:
    // AH_STAGE_REGISTER=1 registers the caller's buffer for the duration of the call (measurement aid).
    const bool try_register = tun(TUN_STAGE_REGISTER) != 0;
    if (try_register && !src.bq && src.fpitch == ds->dims && n * src.frb >= (64u << 20)) {
        Ring ring;
        AH_TRY(upload_context(ds, 0, &t.ctx));
        AH_TRY(ring_for(&t, 1, nullptr, pad256(std::min<size_t>(n, kStageBytes / 4) * 4), &ring));
        Context *ctx = t.ctx;
        if (hipHostRegister(const_cast<float *>(vectors), n * src.frb, hipHostRegisterDefault) == hipSuccess) {
            const uint64_t row0 = ds->n;
            hipError_t e = hipMemcpyAsync(ds->d_rows_f32 + row0 * ds->pitch, vectors, n * src.frb, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(ds->d_ids + row0, item_ids, n * 4, hipMemcpyHostToDevice, ctx->stream);
            int st = e == hipSuccess ? launch_headers_from_vectors(ds->view(), row0, n, ctx->stream) : AH_ERR_DEVICE;
            const hipError_t es = hipStreamSynchronize(ctx->stream);  // the caller's pages are the DMA source
            (void)hipHostUnregister(const_cast<float *>(vectors));
            AH_REQUIRE(e == hipSuccess && es == hipSuccess && st == AH_OK, AH_ERR_DEVICE, "registered staging copy failed");
            note_ids(ds, item_ids, n);
            return AH_OK;
        }
        (void)hipGetLastError();  // not registrable: fall through to the bounce path
    }
    const auto t_begin = now();
    StageTimes tm;
    AH_TRY(stage_loop(&t, 1, nullptr, src, ds->n, n, &tm));
    const auto t_loop = now();
    note_ids(ds, item_ids, n);
    if (tun(TUN_TIMING) != 0) report_times(n, ds->dims, 0, tm, secs_between(t_begin, t_loop), secs_between(t_loop, now()));
    return AH_OK;
    AH_GUARDED_END
}

int ah_dataset_upload_flush(ah_dataset *ds) {
    AH_GUARDED("ah_dataset_upload_flush")
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    return upload_flush(ds);
    AH_GUARDED_END
}

int ah_group_upload_vectors(ah_group *g, const uint32_t *item_ids, const float *vectors, size_t n) {
    AH_GUARDED("ah_group_upload_vectors")
    AH_REQUIRE(g, AH_ERR_INVALID_ARGUMENT, "group is NULL");
    AH_TRY(check_ids(g->members[0], item_ids, n));  // (the members are in the same state)
    if (n == 0) return AH_OK;
    AH_REQUIRE(item_ids && vectors, AH_ERR_INVALID_ARGUMENT, "NULL input");
    return group_upload(g, item_ids, vectors, nullptr, n);
    AH_GUARDED_END
}

// LMDB pages -> the group's pinned ring (once) -> every member.
int ah_group_upload_records(ah_group *g, const uint32_t *item_ids, const uint8_t *const *record_ptrs, size_t record_len,
                            size_t n) {
    AH_GUARDED("ah_group_upload_records")
    AH_REQUIRE(g, AH_ERR_INVALID_ARGUMENT, "group is NULL");
    AH_TRY(check_ids(g->members[0], item_ids, n));
    if (n == 0) return AH_OK;
    AH_REQUIRE(item_ids && record_ptrs, AH_ERR_INVALID_ARGUMENT, "NULL input");
    AH_TRY(check_record_len(g->metric, g->dims, record_len));
    return group_upload(g, item_ids, nullptr, record_ptrs, n);
    AH_GUARDED_END
}

int ah_group_upload_flush(ah_group *g) {
    AH_GUARDED("ah_group_upload_flush")
    AH_REQUIRE(g, AH_ERR_INVALID_ARGUMENT, "group is NULL");
    DeviceRestore restore_device;
    return flush_staging(g);
    AH_GUARDED_END
}

}  // extern "C"
