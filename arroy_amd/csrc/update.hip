// update.hip — ah_dataset_update_* / ah_group_update_* (include/arroy_hip.h): the item changes of one `Writer::build`
// (src/writer.rs:497-505: to_delete = updated, to_insert = items & updated) applied to a finalized dataset where it lives,
// so that an incremental build re-sends only the rows that changed instead of staging every item again.
//
// Shape of an update:
//   1. the upserted items are staged into side buffers by the ring, codec and header kernels of ah_dataset_upload_*;
//   2. plan: every old row whose id is removed or upserted leaves; an exclusive scan of the keep flags ranks the others.
//      Kept old row r lands at keep_rank[r] + lower_bound(upsert_ids, id[r]), upserted row j at
//      j + keep_rank[lower_bound(old_ids, upsert_ids[j])];
//   3. move: one streaming copy kernel writes rows, headers and ids into new arrays, a wave per row;
//   4. fast paths without a second row buffer: the id set does not change (upserted rows scattered over their old rows), or
//      every new id is above the last one and the allocation has room (rows written after row n);
//   5. commit: pointers swapped only after every allocation and kernel has succeeded; the derived copies of the rows
//      (binary16, int8, packed) and their latches are dropped, so the next call that wants one rebuilds it from the rows as it
//      would on a fresh dataset.  Every observable is then that of a dataset staged afresh with the resulting items.
#include <algorithm>
#include <chrono>
#include <vector>

#include "common.h"
#include "scan_device.h"

using namespace ah;

namespace {

constexpr unsigned kUpBlock = 256;                          // 4 waves
enum Path { kInPlace = 0, kAppend = 1, kMerge = 2 };
const char *const kPathName[3] = {"in place", "append", "merge"};

__device__ __forceinline__ uint64_t lower_bound_u32(const uint32_t *a, uint64_t n, uint32_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// plan, step 1: keep[r] = 1 unless the id of old row r is removed or upserted; ins[r] = upserted ids below it
__global__ __launch_bounds__(kUpBlock) void k_update_flags(const uint32_t *__restrict__ ids, uint64_t n,
                                                           const uint32_t *__restrict__ rm, uint64_t n_rm,
                                                           const uint32_t *__restrict__ up, uint64_t n_up,
                                                           uint32_t *__restrict__ keep, uint32_t *__restrict__ ins) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint32_t id = ids[r];
        const uint64_t u = lower_bound_u32(up, n_up, id);
        const uint64_t d = lower_bound_u32(rm, n_rm, id);
        const bool leaves = (u < n_up && up[u] == id) || (d < n_rm && rm[d] == id);
        keep[r] = leaves ? 0u : 1u;
        ins[r] = (uint32_t)u;
    }
}

// the row each upserted item goes to: merge: j + the kept old rows below its id; in place: the old row holding its id;
// append: n_old + j
__global__ __launch_bounds__(kUpBlock) void k_upsert_dest(const uint32_t *__restrict__ up, uint64_t n_up,
                                                          const uint32_t *__restrict__ ids, uint64_t n_old,
                                                          const uint32_t *__restrict__ keep_rank, int path,
                                                          uint32_t *__restrict__ dest) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_up; j += stride) {
        uint64_t to = n_old + j;
        if (path != kAppend) {
            const uint64_t p = lower_bound_u32(ids, n_old, up[j]);
            to = path == kInPlace ? p : j + keep_rank[p];
        }
        dest[j] = (uint32_t)to;
    }
}

typedef uint32_t u32x4_v __attribute__((ext_vector_type(4)));

struct MoveArgs {
    // kept old rows (n_old = 0: none): keep_rank has n_old + 1 entries, row r is kept when keep_rank[r + 1] != keep_rank[r]
    const uint8_t *old_rows;
    const float *old_hdr;
    const uint32_t *old_ids;
    const uint32_t *keep_rank, *ins;
    uint64_t n_old;
    // staged rows and where each goes
    const uint8_t *side_rows;
    const float *side_hdr;
    const uint32_t *side_ids, *dest;
    uint64_t n_side;
    uint8_t *rows;
    float *hdr;
    uint32_t *ids;
    uint64_t rb;  // bytes per row, a multiple of 16
    uint32_t hf;  // header floats per row
};

// move: a wave per row, 16 bytes a lane (a 768-d f32 row is three 1 KiB wave loads), streamed past the caches; the row's
// header and id ride along.  Rows of the old dataset first, then the staged ones.
__global__ __launch_bounds__(kUpBlock) void k_move_rows(MoveArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * (kUpBlock / 64);
    const uint64_t total = a.n_old + a.n_side;
    for (uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < total; q += n_waves) {
        const uint8_t *src;
        const float *src_hdr;
        uint32_t id;
        uint64_t to;
        if (q < a.n_old) {
            const uint32_t rank = a.keep_rank[q];
            if (a.keep_rank[q + 1] == rank) continue;  // (wave-uniform)
            to = (uint64_t)rank + a.ins[q];
            src = a.old_rows + q * a.rb;
            src_hdr = a.old_hdr + q * a.hf;
            id = a.old_ids[q];
        } else {
            const uint64_t j = q - a.n_old;
            to = a.dest[j];
            src = a.side_rows + j * a.rb;
            src_hdr = a.side_hdr + j * a.hf;
            id = a.side_ids[j];
        }
        uint8_t *dst = a.rows + to * a.rb;
        for (uint64_t c = (uint64_t)lane * 16; c < a.rb; c += 64 * 16) {
            const u32x4_v v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_v *>(src + c));
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4_v *>(dst + c));
        }
        if (lane < a.hf) a.hdr[to * a.hf + lane] = src_hdr[lane];
        if (lane == 0) a.ids[to] = id;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

struct UpdateArgs {
    const uint32_t *rm;
    size_t n_rm;
    const uint32_t *up;
    size_t n_up;
    const float *vectors;          // ah_*_update_vectors
    const uint8_t *const *records;  // ah_*_update_records
};

// What the dataset looks like afterwards, from the host mirror of its ids (the same for every member of a group).
struct Plan {
    Path path = kInPlace;
    uint64_t n_old = 0, n_new = 0, cap_new = 0;
    uint32_t last_id = 0;
    bool identity = true;
    uint32_t lut_len = 0;  // 0: no id -> row table (identity ids, or too sparse: the kernels binary-search the ids)
};

// the ids of the dataset as a sorted array (an identity dataset staged by ah_dataset_fill_synthetic keeps no host mirror)
const uint32_t *old_ids_of(const ah_dataset *ds, std::vector<uint32_t> *iota) {
    if (ds->h_ids.size() == ds->n) return ds->h_ids.data();
    iota->resize(ds->n);
    for (uint64_t i = 0; i < ds->n; i++) (*iota)[i] = (uint32_t)i;
    return iota->data();
}

int check_sorted(const uint32_t *ids, size_t n, const char *what) {
    AH_REQUIRE(ids || n == 0, AH_ERR_INVALID_ARGUMENT, "%s is NULL", what);
    for (size_t i = 1; i < n; i++)
        AH_REQUIRE(ids[i] > ids[i - 1], AH_ERR_INVALID_ARGUMENT, "%s must be strictly ascending (id %u after %u)", what, ids[i],
                   ids[i - 1]);
    return AH_OK;
}

int check_member(ah_dataset *ds) {
    AH_REQUIRE(ds->finalized, AH_ERR_NOT_FINALIZED, "dataset not finalized (an update applies to a finalized dataset)");
    AH_REQUIRE(ds->live_indexes.load(std::memory_order_acquire) == 0, AH_ERR_INVALID_ARGUMENT,
               "an ah_index built on the dataset is alive (%d): it holds row positions; destroy it before the update",
               ds->live_indexes.load(std::memory_order_relaxed));
    return AH_OK;
}

int check_record_len(int metric, uint32_t dims, size_t record_len) {
    const size_t hs = ah_header_size(metric), vs = ah_vector_size(metric, dims);
    if (record_len != 1 + hs + vs) {
        set_error("record length %zu does not match 1 + %zu + %zu for %u dimensions", record_len, hs, vs, dims);
        set_error_status(AH_ERR_INVALID_DIMENSION);
        set_error_detail(0, 1 + hs + vs, record_len);
        return AH_ERR_INVALID_DIMENSION;
    }
    return AH_OK;
}

Plan make_plan(const ah_dataset *ds, const UpdateArgs &a) {
    Plan p;
    std::vector<uint32_t> iota;
    const uint32_t *old = old_ids_of(ds, &iota);
    const uint64_t n = ds->n;
    auto present = [&](uint32_t id) { return std::binary_search(old, old + n, id); };
    uint64_t leaving = 0;
    bool all_up_present = true, any_rm_leaves = false;
    for (size_t j = 0; j < a.n_up; j++) {
        if (present(a.up[j])) leaving++;
        else all_up_present = false;
    }
    for (size_t i = 0; i < a.n_rm; i++)
        if (present(a.rm[i]) && !std::binary_search(a.up, a.up + a.n_up, a.rm[i])) {
            leaving++;
            any_rm_leaves = true;
        }
    p.n_old = n;
    p.n_new = n - leaving + a.n_up;
    const uint64_t allocated = std::max<uint64_t>(ds->capacity, 1);
    if (all_up_present && !any_rm_leaves) p.path = kInPlace;  // the id set does not change
    else if (!any_rm_leaves && (n == 0 || a.up[0] > old[n - 1]) && p.n_new <= allocated) p.path = kAppend;
    else p.path = kMerge;
    p.cap_new = p.path == kMerge ? std::max<uint64_t>(p.n_new, ds->capacity) : ds->capacity;
    if (p.path == kInPlace) {
        p.last_id = ds->last_id;
    } else {
        // the larger of the last upserted id and the largest old id that stays
        p.last_id = a.n_up ? a.up[a.n_up - 1] : 0;
        for (uint64_t r = n; r-- > 0 && old[r] > p.last_id;)
            if (!std::binary_search(a.up, a.up + a.n_up, old[r]) && !std::binary_search(a.rm, a.rm + a.n_rm, old[r])) {
                p.last_id = old[r];
                break;
            }
    }
    // what ah_dataset_finalize derives for these ids (note_ids: identity means ids 0 .. n - 1)
    p.identity = p.path == kInPlace ? ds->identity_ids : (p.n_new == 0 || (uint64_t)p.last_id == p.n_new - 1);
    if (!p.identity) {
        const uint64_t span = (uint64_t)p.last_id + 1;
        if (span <= 8 * p.n_new + (1u << 20)) p.lut_len = (uint32_t)span;
    }
    return p;
}

// the new host mirror of the ids: the old ids that stay merged with the upserted ones
void merge_ids(const ah_dataset *ds, const UpdateArgs &a, const Plan &p, std::vector<uint32_t> *out) {
    std::vector<uint32_t> iota;
    const uint32_t *old = old_ids_of(ds, &iota);
    out->clear();
    out->reserve(p.n_new);
    if (p.path == kAppend) {
        out->insert(out->end(), old, old + p.n_old);
        out->insert(out->end(), a.up, a.up + a.n_up);
        return;
    }
    size_t j = 0, d = 0;
    for (uint64_t r = 0; r < p.n_old; r++) {
        const uint32_t id = old[r];
        while (j < a.n_up && a.up[j] < id) out->push_back(a.up[j++]);
        while (d < a.n_rm && a.rm[d] < id) d++;
        if ((j < a.n_up && a.up[j] == id) || (d < a.n_rm && a.rm[d] == id)) continue;
        out->push_back(id);
    }
    while (j < a.n_up) out->push_back(a.up[j++]);
}

int alloc(DevMem *m, size_t bytes) { return ah::alloc(m, bytes, "the update"); }

// One member's share of an update: everything it allocates before the commit, owned until then.
struct MemberUpdate {
    ah_dataset *ds = nullptr;
    ContextLease *lease = nullptr;
    DevMem side_rows, side_hdr, side_ids;   // the staged upserts
    DevMem rm, keep_rank, ins, tile_sums, dest;
    DevMem rows, hdr, ids;                  // merge: the new arrays
    DevMem lut;                             // the new id -> row table (not in place)
    std::vector<uint32_t> h_ids;            // the new host mirror (not in place)
    MemberUpdate() = default;
    MemberUpdate(const MemberUpdate &) = delete;
    ~MemberUpdate() { delete lease; }
    StageDst side() const { return StageDst{side_rows.as<uint8_t>(), side_hdr.as<float>(), side_ids.as<uint32_t>()}; }
};

// phase 1: the member's buffers and stream
int prepare(MemberUpdate *mu, const Plan &p, const UpdateArgs &a) {
    ah_dataset *ds = mu->ds;
    AH_HIP(hipSetDevice(ds->device));
    mu->lease = new ContextLease(ds);
    AH_REQUIRE(mu->lease->c, AH_ERR_DEVICE, "cannot create a HIP stream");
    const size_t rb = ds->row_bytes(), hs = ah_header_size(ds->metric);
    if (a.n_up) {
        AH_TRY(alloc(&mu->side_rows, a.n_up * rb));
        AH_TRY(alloc(&mu->side_hdr, a.n_up * hs));
        AH_TRY(alloc(&mu->side_ids, a.n_up * 4));
        AH_TRY(alloc(&mu->dest, a.n_up * 4));
    }
    if (p.path == kMerge) {
        const uint64_t nb = (p.n_old + kScanTile - 1) / kScanTile;
        AH_TRY(alloc(&mu->rm, a.n_rm * 4));
        AH_TRY(alloc(&mu->keep_rank, (p.n_old + 1) * 4));
        AH_TRY(alloc(&mu->ins, p.n_old * 4));
        AH_TRY(alloc(&mu->tile_sums, nb * 4));
        const uint64_t cap = std::max<uint64_t>(p.cap_new, 1);
        AH_TRY(alloc(&mu->rows, cap * rb));
        AH_TRY(alloc(&mu->hdr, cap * hs));
        AH_TRY(alloc(&mu->ids, cap * 4));
    }
    if (p.path != kInPlace && p.lut_len) AH_TRY(alloc(&mu->lut, (size_t)p.lut_len * 4));
    return AH_OK;
}

// phase 2 (after the staging): the plan and, for a merge, the move into the new arrays.  Queued on the member's stream.
int launch_plan(MemberUpdate *mu, const Plan &p, const UpdateArgs &a) {
    ah_dataset *ds = mu->ds;
    AH_HIP(hipSetDevice(ds->device));
    const hipStream_t s = mu->lease->c->stream;
    uint32_t *keep_rank = mu->keep_rank.as<uint32_t>();
    if (p.path == kMerge) {
        if (a.n_rm) AH_HIP(hipMemcpyAsync(mu->rm.p, a.rm, a.n_rm * 4, hipMemcpyHostToDevice, s));
        if (p.n_old)
            hipLaunchKernelGGL(k_update_flags, dim3(grid_of(p.n_old, kUpBlock, 1u << 16)), dim3(kUpBlock), 0, s, ds->d_ids, p.n_old,
                               mu->rm.as<const uint32_t>(), (uint64_t)a.n_rm, mu->side_ids.as<const uint32_t>(), (uint64_t)a.n_up,
                               keep_rank, mu->ins.as<uint32_t>());
        launch_exclusive_scan(keep_rank, p.n_old, mu->tile_sums.as<uint32_t>(), keep_rank + p.n_old, s);
    }
    if (a.n_up)
        hipLaunchKernelGGL(k_upsert_dest, dim3(grid_of(a.n_up, kUpBlock, 4096)), dim3(kUpBlock), 0, s, mu->side_ids.as<const uint32_t>(),
                           (uint64_t)a.n_up, ds->d_ids, p.n_old, keep_rank, (int)p.path, mu->dest.as<uint32_t>());
    if (p.path == kMerge) {
        MoveArgs m{};
        m.old_rows = own_dst(ds).rows;
        m.old_hdr = ds->d_headers;
        m.old_ids = ds->d_ids;
        m.keep_rank = keep_rank;
        m.ins = mu->ins.as<const uint32_t>();
        m.n_old = p.n_old;
        m.side_rows = mu->side_rows.as<const uint8_t>();
        m.side_hdr = mu->side_hdr.as<const float>();
        m.side_ids = mu->side_ids.as<const uint32_t>();
        m.dest = mu->dest.as<const uint32_t>();
        m.n_side = a.n_up;
        m.rows = mu->rows.as<uint8_t>();
        m.hdr = mu->hdr.as<float>();
        m.ids = mu->ids.as<uint32_t>();
        m.rb = ds->row_bytes();
        m.hf = header_floats(ds->metric);
        if (p.n_old + a.n_up)
            hipLaunchKernelGGL(k_move_rows, dim3(grid_of(p.n_old + a.n_up, kUpBlock / 64, 8192)), dim3(kUpBlock), 0, s, m);
        if (p.lut_len) AH_TRY(launch_build_lut(mu->ids.as<const uint32_t>(), p.n_new, mu->lut.as<uint32_t>(), p.lut_len, s));
    }
    AH_HIP(hipGetLastError());
    return AH_OK;
}

// phase 3, once every member has come through phases 1 and 2: the staged rows written into the dataset's own arrays (in
// place / append), the new table built
int launch_write(MemberUpdate *mu, const Plan &p, const UpdateArgs &a) {
    if (p.path == kMerge) return AH_OK;
    ah_dataset *ds = mu->ds;
    AH_HIP(hipSetDevice(ds->device));
    const hipStream_t s = mu->lease->c->stream;
    if (a.n_up) {
        MoveArgs m{};
        m.side_rows = mu->side_rows.as<const uint8_t>();
        m.side_hdr = mu->side_hdr.as<const float>();
        m.side_ids = mu->side_ids.as<const uint32_t>();
        m.dest = mu->dest.as<const uint32_t>();
        m.n_side = a.n_up;
        const StageDst own = own_dst(ds);
        m.rows = own.rows;
        m.hdr = own.headers;
        m.ids = own.ids;
        m.rb = ds->row_bytes();
        m.hf = header_floats(ds->metric);
        hipLaunchKernelGGL(k_move_rows, dim3(grid_of(a.n_up, kUpBlock / 64, 8192)), dim3(kUpBlock), 0, s, m);
    }
    if (p.path == kAppend && p.lut_len) AH_TRY(launch_build_lut(ds->d_ids, p.n_new, mu->lut.as<uint32_t>(), p.lut_len, s));
    AH_HIP(hipGetLastError());
    return AH_OK;
}

template <typename T>
void free_copy(T *&p) {
    if (p) (void)dev_free(p);
    p = nullptr;
}

// phase 4: the new state is published (nothing here can fail)
void commit(MemberUpdate *mu, const Plan &p) {
    ah_dataset *ds = mu->ds;
    (void)hipSetDevice(ds->device);
    std::lock_guard<std::mutex> lk(ds->mu);
    // (the old arrays go into the DevMems, which free them)
    if (p.path == kMerge) {
        const StageDst old = own_dst(ds);
        if (metric_is_bq(ds->metric)) ds->d_rows_bq = mu->rows.as<uint64_t>();
        else ds->d_rows_f32 = mu->rows.as<float>();
        ds->d_headers = mu->hdr.as<float>();
        ds->d_ids = mu->ids.as<uint32_t>();
        mu->rows.p = old.rows;
        mu->hdr.p = old.headers;
        mu->ids.p = old.ids;
        ds->capacity = p.cap_new;
    }
    if (p.path != kInPlace) {
        uint32_t *old_lut = ds->d_lut;
        ds->d_lut = mu->lut.as<uint32_t>();
        mu->lut.p = old_lut;
        ds->lut_len = p.lut_len;
        ds->h_ids.swap(mu->h_ids);
        ds->n = p.n_new;
        ds->last_id = p.last_id;
        ds->identity_ids = p.identity;
    }
    // the copies derived from the rows, and every decision taken about them: rebuilt on demand as on a fresh dataset
    ds->screen_ready.store(false, std::memory_order_release);
    ds->screen8_ready.store(false, std::memory_order_release);
    ds->packed_ready.store(false, std::memory_order_release);
    free_copy(ds->d_rows_h16);
    free_copy(ds->d_screen_stats);
    free_copy(ds->d_rows_i8);
    free_copy(ds->d_rows_i8_lo);
    free_copy(ds->d_scale8_rows);
    free_copy(ds->d_dim_scale);
    free_copy(ds->d_packed);
    free_copy(ds->d_packed_exp);
    std::fill(std::begin(ds->screen_max), std::end(ds->screen_max), 0.0f);
    std::fill(std::begin(ds->screen8_max), std::end(ds->screen8_max), 0.0f);
    ds->hpitch = 0;
    ds->pitch8 = 0;
    ds->screen8_quality = 0.0;
    ds->screen_never = false;
    ds->screen8_decided = false;
    ds->screen_alloc_failed = false;
    ds->packed_raw_rows = 0;
    ds->packed_grid_rows = 0;
    ds->packed_decided.store(false, std::memory_order_release);
    ds->rerank8_fails.store(0, std::memory_order_relaxed);
    ds->rerank8_seen.store(0, std::memory_order_relaxed);
    ds->rerank8_off.store(false, std::memory_order_relaxed);
    ds->rr_stats = ah_rerank_stats{};
    // DotProduct: the headers of the upserted rows are {0, 0} (or whatever the records held) and the max norm may have
    // changed: preprocess again (src/writer.rs:964-976 does so inside every build)
    if (ds->metric == AH_DOT_PRODUCT) ds->dot_preprocessed = false;
    ds->update_fast_paths[p.path]++;
}

// The whole update over `members` (one dataset, or every member of a group): all or nothing.
int update_impl(const std::vector<ah_dataset *> &members, ah_group *g, const UpdateArgs &a) {
    auto now = [] { return std::chrono::steady_clock::now(); };
    const auto t0 = now();
    ah_dataset *ds0 = members[0];
    for (ah_dataset *m : members) {
        AH_TRY(flush_staging(m));
        AH_TRY(check_member(m));
    }
    AH_TRY(check_sorted(a.rm, a.n_rm, "remove_ids"));
    AH_TRY(check_sorted(a.up, a.n_up, "upsert_ids"));
    AH_REQUIRE(a.n_up == 0 || a.vectors || a.records, AH_ERR_INVALID_ARGUMENT, "the upserted items are NULL");
    const Plan p = make_plan(ds0, a);
    AH_REQUIRE(p.n_new < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT, "the update exceeds the u32 item-id space");
    DeviceRestore restore_device;
    std::vector<MemberUpdate> mus(members.size());
    for (size_t i = 0; i < members.size(); i++) mus[i].ds = members[i];
    for (MemberUpdate &mu : mus) AH_TRY(prepare(&mu, p, a));
    const auto t_alloc = now();
    // the upserted rows cross PCIe once: into every member's side buffers through the dataset's (the group's) pinned ring
    // (stage.hip), and have landed when the call returns
    if (a.n_up) {
        std::vector<StageDst> dst;
        for (MemberUpdate &mu : mus) dst.push_back(mu.side());
        AH_TRY(stage_items(members, g, dst.data(), a.up, a.vectors, a.records, a.n_up));
    }
    const auto t_stage = now();
    for (MemberUpdate &mu : mus) AH_TRY(launch_plan(&mu, p, a));
    // the host mirror of the ids is merged while the devices move the rows
    if (p.path != kInPlace) {
        merge_ids(ds0, a, p, &mus[0].h_ids);
        for (size_t i = 1; i < mus.size(); i++) mus[i].h_ids = mus[0].h_ids;
    }
    for (MemberUpdate &mu : mus) {
        AH_HIP(hipSetDevice(mu.ds->device));
        AH_HIP(hipStreamSynchronize(mu.lease->c->stream));
    }
    const auto t_plan = now();
    for (MemberUpdate &mu : mus) AH_TRY(launch_write(&mu, p, a));
    for (MemberUpdate &mu : mus) {
        AH_HIP(hipSetDevice(mu.ds->device));
        AH_HIP(hipStreamSynchronize(mu.lease->c->stream));
    }
    {
        NoFailScope no_fail;
        for (MemberUpdate &mu : mus) commit(&mu, p);
    }
    if (tun(TUN_TIMING) != 0) {
        auto secs = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) {
            return std::chrono::duration<double>(y - x).count();
        };
        fprintf(stderr, "[ah] update %s: %llu -> %llu rows (%zu removed, %zu upserted ids) on %zu dataset(s): buffers %.4f s, staging %.4f s, "
                        "plan + move %.4f s, write + commit %.4f s\n",
                kPathName[p.path], (unsigned long long)p.n_old, (unsigned long long)p.n_new, a.n_rm, a.n_up, members.size(),
                secs(t0, t_alloc), secs(t_alloc, t_stage), secs(t_stage, t_plan), secs(t_plan, now()));
    }
    return AH_OK;
}

}  // namespace

extern "C" {

int ah_dataset_update_vectors(ah_dataset *ds, const uint32_t *remove_ids, size_t n_remove, const uint32_t *upsert_ids,
                              const float *vectors, size_t n_upsert) {
    AH_GUARDED("ah_dataset_update_vectors")
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    AH_REQUIRE(!ds->group_member, AH_ERR_INVALID_ARGUMENT, "the dataset is a member of a device group: use ah_group_update_vectors");
    AH_REQUIRE(vectors || n_upsert == 0, AH_ERR_INVALID_ARGUMENT, "vectors is NULL");
    const UpdateArgs a{remove_ids, n_remove, upsert_ids, n_upsert, vectors, nullptr};
    return update_impl({ds}, nullptr, a);
    AH_GUARDED_END
}

int ah_dataset_update_records(ah_dataset *ds, const uint32_t *remove_ids, size_t n_remove, const uint32_t *upsert_ids,
                              const uint8_t *const *record_ptrs, size_t record_len, size_t n_upsert) {
    AH_GUARDED("ah_dataset_update_records")
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    AH_REQUIRE(!ds->group_member, AH_ERR_INVALID_ARGUMENT, "the dataset is a member of a device group: use ah_group_update_records");
    AH_REQUIRE(record_ptrs || n_upsert == 0, AH_ERR_INVALID_ARGUMENT, "record_ptrs is NULL");
    if (n_upsert) AH_TRY(check_record_len(ds->metric, ds->dims, record_len));
    const UpdateArgs a{remove_ids, n_remove, upsert_ids, n_upsert, nullptr, record_ptrs};
    return update_impl({ds}, nullptr, a);
    AH_GUARDED_END
}

int ah_group_update_vectors(ah_group *group, const uint32_t *remove_ids, size_t n_remove, const uint32_t *upsert_ids,
                            const float *vectors, size_t n_upsert) {
    AH_GUARDED("ah_group_update_vectors")
    AH_REQUIRE(group, AH_ERR_INVALID_ARGUMENT, "group is NULL");
    AH_REQUIRE(vectors || n_upsert == 0, AH_ERR_INVALID_ARGUMENT, "vectors is NULL");
    const UpdateArgs a{remove_ids, n_remove, upsert_ids, n_upsert, vectors, nullptr};
    return update_impl(group->members, group, a);
    AH_GUARDED_END
}

int ah_group_update_records(ah_group *group, const uint32_t *remove_ids, size_t n_remove, const uint32_t *upsert_ids,
                            const uint8_t *const *record_ptrs, size_t record_len, size_t n_upsert) {
    AH_GUARDED("ah_group_update_records")
    AH_REQUIRE(group, AH_ERR_INVALID_ARGUMENT, "group is NULL");
    AH_REQUIRE(record_ptrs || n_upsert == 0, AH_ERR_INVALID_ARGUMENT, "record_ptrs is NULL");
    if (n_upsert) AH_TRY(check_record_len(group->metric, group->dims, record_len));
    const UpdateArgs a{remove_ids, n_remove, upsert_ids, n_upsert, nullptr, record_ptrs};
    return update_impl(group->members, group, a);
    AH_GUARDED_END
}

int ah_debug_update_paths(ah_dataset *ds, uint64_t *out_in_place, uint64_t *out_appended, uint64_t *out_merged) {
    AH_GUARDED("ah_debug_update_paths")
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    std::lock_guard<std::mutex> lk(ds->mu);
    if (out_in_place) *out_in_place = ds->update_fast_paths[kInPlace];
    if (out_appended) *out_appended = ds->update_fast_paths[kAppend];
    if (out_merged) *out_merged = ds->update_fast_paths[kMerge];
    return AH_OK;
    AH_GUARDED_END
}

}  // extern "C"
