// index_encode.hip — ah_index_encode_nodes (include/arroy_hip.h): the nodes of a resident index as the `NodeCodec` values LMDB
// stores for them (node_codec.h), encoded where the index lives.  The inverse of index_decode.hip; the Descendants half is
// encode.hip's, reached through the launchers of encode.h.
//
//   gather    one thread per listed node: the DNode is validated (index in range, not free, children in use, list and normal
//             row inside the index's arrays, ids within 32 bits) and becomes an EncNode — Descendants: byte offset into d_desc
//             and count; split: the normal row and the two children as the STORE's ids — plus its info word (0 / kEncInfoSplit
//             / kEncInfoFree) and, for everything but a Descendants node, its value length.  The first offender by list
//             position is kept with one 64-bit atomicMin.
//   measure   encode.hip's wave-per-list measure fills in the Descendants lengths, then ONE 64-bit exclusive scan runs over
//             the mixed sequence (launch_measure_mixed).
//   write     piece by piece — whole values that fit half of the pinned read-back buffer (AH_READBACK_MB), a longer value
//             alone: Descendants through encode.hip's writers, which skip the other info words; split values through
//             k_ixenc_write_split, a wavefront per node.  A split value's body is the word stream [header words][vector
//             words] of the index's own normal arrays shifted by the value's 9-byte head, so once the destination is on a
//             4-byte boundary lane i stores the aligned word i, funnel-shifted out of source words q and q + 1: consecutive
//             lanes read consecutive words of the row and write consecutive words of the value.  The bytes in front of the
//             boundary and behind the last whole word are byte stores, as in k_enc_write_split.
//
// Every pass reads the index and writes scratch only; nothing is written to the caller's buffer before every refusal is
// through.  Scratch: 28 bytes per listed node (+ 4 per listed index, + 4 per node slot with an id table) and two device /
// pinned halves of a piece — never the total of the values.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "encode.h"
#include "index_device.h"
#include "node_codec.h"

using namespace ah;

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kIxEncBlock = 256;

enum IxEncBad : uint32_t { BAD_INDEX = 0, BAD_FREE, BAD_CHILD, BAD_ID, BAD_NODE };

struct IxEncCtl {
    unsigned long long first_bad;  // list position << 3 | IxEncBad of the first offender; all ones: none
    uint32_t enc_err;              // kEncErr* / kEncHasBitmap of the measure
    uint32_t n_split, n_desc, n_free;
};

struct GatherArgs {
    const DNode *nodes;
    uint32_t n_nodes, n_normals;
    uint64_t desc_len;
    const uint32_t *list;   // nullptr: every slot
    const uint32_t *id_of;  // nullptr: base + slot
    uint32_t base;
    uint32_t split_len;     // a split value with a normal
    EncNode *out;
    uint64_t *len;
    uint32_t *info;
    IxEncCtl *ctl;
};

__device__ __forceinline__ bool store_id(const GatherArgs &a, uint32_t slot, uint32_t *id) {
    if (a.id_of) {
        *id = a.id_of[slot];
        return true;
    }
    const uint64_t v = (uint64_t)a.base + slot;
    *id = (uint32_t)v;
    return v <= 0xFFFFFFFFull;
}

__global__ __launch_bounds__(kIxEncBlock) void k_ixenc_gather(GatherArgs a, uint64_t n) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t stride = (uint64_t)gridDim.x * kIxEncBlock;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kIxEncBlock + (threadIdx.x & ~(kWave - 1)); i0 < n; i0 += stride) {  // (wave-uniform)
        const uint64_t i = i0 + lane;
        const bool active = i < n;
        uint32_t bad = 0xFFFFFFFFu, info = kEncInfoFree;
        uint64_t len = 0;
        EncNode e{0, 0, 0};
        bool is_split = false, is_desc = false, is_free = false;
        if (active) {
            const uint32_t slot = a.list ? a.list[i] : (uint32_t)i;
            if (slot >= a.n_nodes) {
                bad = BAD_INDEX;
            } else {
                const DNode d = a.nodes[slot];
                const uint32_t kind = d.kind & 0xFFu;
                uint32_t own = 0;
                if (kind == 0) {
                    is_free = true;
                    if (a.list) bad = BAD_FREE;
                } else if (!store_id(a, slot, &own)) {
                    bad = BAD_ID;
                } else if (kind == AH_NODE_DESCENDANTS) {
                    is_desc = true;
                    info = 0;
                    e = EncNode{(uint64_t)d.a * 4, d.b, 0u};
                    if ((uint64_t)d.a + d.b > a.desc_len) bad = BAD_NODE;
                } else if (kind == AH_NODE_SPLIT) {
                    is_split = true;
                    info = kEncInfoSplit;
                    const bool has_normal = (d.kind & 0x100u) != 0;
                    len = has_normal ? a.split_len : codec::kSplitHead;
                    uint32_t l = 0, r = 0;
                    if (d.a >= a.n_nodes || d.b >= a.n_nodes || (a.nodes[d.a].kind & 0xFFu) == 0 || (a.nodes[d.b].kind & 0xFFu) == 0) bad = BAD_CHILD;
                    else if (!store_id(a, d.a, &l) || !store_id(a, d.b, &r)) bad = BAD_ID;
                    else if (has_normal && d.c >= a.n_normals) bad = BAD_NODE;
                    e = EncNode{has_normal ? d.c : 0u, l, r};
                } else {
                    bad = BAD_NODE;
                }
            }
            if (bad != 0xFFFFFFFFu) {  // nothing of an offender is read later: an empty value
                atomicMin(&a.ctl->first_bad, ((unsigned long long)i << 3) | bad);
                e = EncNode{0, 0, 0};
                info = kEncInfoFree;
                len = 0;
            }
            a.out[i] = e;
            a.info[i] = info;
            a.len[i] = len;  // (a Descendants node: the measure's)
        }
        const uint64_t m_split = __ballot(is_split), m_desc = __ballot(is_desc), m_free = __ballot(is_free);
        if (lane == 0) {
            if (m_split) atomicAdd(&a.ctl->n_split, (uint32_t)__popcll(m_split));
            if (m_desc) atomicAdd(&a.ctl->n_desc, (uint32_t)__popcll(m_desc));
            if (m_free) atomicAdd(&a.ctl->n_free, (uint32_t)__popcll(m_free));
        }
    }
}

// nodes [0, n) of a piece whose info word says split: [2][BE left][BE right] and, for off[i + 1] - off[i] > 9, the header words
// of row nodes[i].src followed by the first `body_words - hf` words of its vector row.
__global__ __launch_bounds__(kIxEncBlock) void k_ixenc_write_split(const EncNode *__restrict__ nodes, const uint32_t *__restrict__ info, uint64_t n,
                                                                  const uint64_t *__restrict__ off, uint64_t out_base, uint8_t *__restrict__ out,
                                                                  const uint32_t *__restrict__ rows, uint32_t row_words32,
                                                                  const uint32_t *__restrict__ hdrs, uint32_t hf) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t n_waves = (uint64_t)gridDim.x * (kIxEncBlock / kWave);
    for (uint64_t node = ((uint64_t)blockIdx.x * kIxEncBlock + threadIdx.x) / kWave; node < n; node += n_waves) {
        if (info[node] != kEncInfoSplit) continue;
        const EncNode nd = nodes[node];
        const uint64_t begin = off[node];
        const uint32_t len = (uint32_t)(off[node + 1] - begin);
        uint8_t *dst = out + (begin - out_base);
        const uint32_t *hdr = hdrs + nd.src * hf, *vec = rows + nd.src * row_words32;  // (read only where len > 9)
        auto body_word = [&](uint32_t q) { return q < hf ? hdr[q] : vec[q - hf]; };
        auto byte_at = [&](uint32_t j) -> uint32_t {
            if (j == 0) return codec::kTagSplit;
            if (j < 5) return (nd.a >> (8 * (4 - j))) & 0xFFu;
            if (j < codec::kSplitHead) return (nd.b >> (8 * (8 - j))) & 0xFFu;
            const uint32_t p = j - codec::kSplitHead;
            return (body_word(p >> 2) >> (8 * (p & 3u))) & 0xFFu;
        };
        // bytes up to the first 4-byte boundary of the destination, aligned words, bytes again
        const uint32_t head = min(len, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
        const uint32_t words = (len - head) / 4;
        if (lane < head) dst[lane] = (uint8_t)byte_at(lane);
        for (uint32_t w = lane; w < words; w += kWave) {
            const uint32_t j = head + 4 * w;
            uint32_t v;
            if (j >= codec::kSplitHead) {  // bytes p .. p + 3 of the body: out of words q and, unless p is a multiple of 4, q + 1
                const uint32_t p = j - codec::kSplitHead, q = p >> 2, sh = 8 * (p & 3u);
                v = body_word(q);
                if (sh) v = (v >> sh) | (body_word(q + 1) << (32 - sh));  // (p + 3 < body bytes: word q + 1 exists)
            } else {
                v = byte_at(j) | byte_at(j + 1) << 8 | byte_at(j + 2) << 16 | byte_at(j + 3) << 24;
            }
            *reinterpret_cast<uint32_t *>(dst + j) = v;
        }
        const uint32_t j = head + 4 * words + lane;
        if (j < len) dst[j] = (uint8_t)byte_at(j);
    }
}

int alloc(DevMem *m, size_t bytes) { return ah::alloc(m, bytes, "the index encode"); }

int encode_nodes_impl(ah_index *ix, const uint32_t *list, size_t n_listed, const uint32_t *id_of, uint32_t base, uint8_t *out, uint64_t out_cap,
                      uint64_t *out_off, ah_index_encode_stats *out_stats) {
    ah_dataset *ds = ix->ds;
    const uint64_t n = list ? (uint64_t)n_listed : ix->n_nodes;
    ah_index_encode_stats st{};
    out_off[0] = 0;
    if (n == 0) {
        if (out_stats) *out_stats = st;
        return AH_OK;
    }
    IndexCall call;
    AH_TRY(call.begin(ds));
    const hipStream_t s = call.stream();
    Context *ctx = call.lease->c;
    const uint32_t hf = header_floats(ds->metric);
    const uint32_t vec_words = (uint32_t)(ah_vector_size(ds->metric, ds->dims) / 4);
    const uint32_t row_words32 = (uint32_t)(ds->row_bytes() / 4);
    AH_REQUIRE(vec_words <= row_words32, AH_ERR_DEVICE, "the normal rows are narrower than a vector");

    // ---- gather, measure, scan: the lengths of every value and every refusal
    DevMem d_list, d_idof, d_nodes, d_off, d_info, d_sums, d_ctl;
    if (list) AH_TRY(alloc(&d_list, (size_t)n * 4));
    if (id_of) AH_TRY(alloc(&d_idof, (size_t)ix->n_nodes * 4));
    AH_TRY(alloc(&d_nodes, (size_t)n * sizeof(EncNode)));
    AH_TRY(alloc(&d_off, (size_t)(n + 1) * 8));
    AH_TRY(alloc(&d_info, (size_t)n * 4));
    AH_TRY(alloc(&d_sums, enc_scan_sums(n) * 8));
    AH_TRY(alloc(&d_ctl, sizeof(IxEncCtl)));
    if (list) AH_HIP(hipMemcpyAsync(d_list.p, list, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (id_of && ix->n_nodes) AH_HIP(hipMemcpyAsync(d_idof.p, id_of, (size_t)ix->n_nodes * 4, hipMemcpyHostToDevice, s));
    IxEncCtl ctl{};
    ctl.first_bad = ~0ull;
    AH_HIP(hipMemcpyAsync(d_ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    GatherArgs g{};
    g.nodes = ix->d_nodes;
    g.n_nodes = ix->n_nodes;
    g.n_normals = ix->n_normals;
    g.desc_len = ix->desc_len;
    g.list = list ? d_list.as<const uint32_t>() : nullptr;
    g.id_of = id_of ? d_idof.as<const uint32_t>() : nullptr;
    g.base = base;
    g.split_len = (uint32_t)codec::split_value_len(true, 4ull * hf, 4ull * vec_words);
    g.out = d_nodes.as<EncNode>();
    g.len = d_off.as<uint64_t>();
    g.info = d_info.as<uint32_t>();
    g.ctl = d_ctl.as<IxEncCtl>();
    hipLaunchKernelGGL(k_ixenc_gather, dim3(grid_of(n, kIxEncBlock, 4096)), dim3(kIxEncBlock), 0, s, g, n);
    AH_HIP(hipGetLastError());
    const uint8_t *src = reinterpret_cast<const uint8_t *>(ix->d_desc);
    AH_TRY(launch_measure_mixed(src, g.out, n, g.len, g.info, d_sums.as<uint64_t>(), &g.ctl->enc_err, s));
    AH_HIP(hipMemcpyAsync(&ctl, d_ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    if (ctl.first_bad != ~0ull) {
        const uint64_t pos = ctl.first_bad >> 3;
        const uint32_t slot = list ? list[pos] : (uint32_t)pos;
        const unsigned long long p = pos;
        switch ((uint32_t)(ctl.first_bad & 7u)) {
            case BAD_INDEX:
                AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "node_indices[%llu] = %u: the index has %u node slots", p, slot, ix->n_nodes);
            case BAD_FREE:
                AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "node_indices[%llu] = %u is a free slot", p, slot);
            case BAD_CHILD:
                AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "node %u (position %llu) has a child that is a free slot or no node slot", slot, p);
            case BAD_ID:
                AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "node %u (position %llu): an id passes 2^32 - 1 with node_id_base %u", slot, p, base);
            default:
                AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT,
                           "node %u (position %llu) is of no known kind, or its list or normal row lies outside the index (ah_index_audit)", slot, p);
        }
    }
    AH_REQUIRE(!(ctl.enc_err & kEncErrOrder), AH_ERR_INVALID_ARGUMENT,
               "a Descendants list of the index does not ascend strictly (ah_index_audit names it)");
    AH_HIP(hipMemcpyAsync(out_off, d_off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    const uint64_t total = out_off[n];
    st.n_values = n;
    st.n_split = ctl.n_split;
    st.n_descendants = ctl.n_desc;
    st.n_free = ctl.n_free;
    st.value_bytes = total;
    if (out && total) {
        AH_REQUIRE(total <= out_cap, AH_ERR_INVALID_ARGUMENT, "the values need %llu bytes, out_cap is %llu", (unsigned long long)total,
                   (unsigned long long)out_cap);
        // ---- write: pieces of whole values, each at most one half of the read-back buffer unless a single value is longer
        uint64_t longest = 0;
        for (uint64_t i = 0; i < n; i++) longest = std::max(longest, out_off[i + 1] - out_off[i]);
        const uint64_t half_mb = (uint64_t)std::min<long long>(4096, std::max<long long>(2, tun(TUN_READBACK_MB))) << 19;
        // (a call for a handful of put nodes takes what its values need, not the whole read-back buffer)
        const size_t half = (size_t)((std::max(std::min(half_mb, total), longest) + 255) & ~255ull);
        DevMem d_out;
        AH_TRY(alloc(&d_out, 2 * half));
        AH_TRY(ctx->ensure_pinned(2 * half));
        uint8_t *pin = reinterpret_cast<uint8_t *>(ctx->h_pinned);
        const hipEvent_t ev[2] = {ctx->ev0, ctx->ev1};
        const bool any_bitmap = (ctl.enc_err & kEncHasBitmap) != 0;
        struct Piece {
            uint64_t at = 0, len = 0;
            int buf = 0;
            bool live = false;
        } prev;
        auto hand_over = [&](const Piece &p) -> int {
            AH_HIP(hipEventSynchronize(ev[p.buf]));
            memcpy(out + p.at, pin + (size_t)p.buf * half, (size_t)p.len);
            return AH_OK;
        };
        int b = 0;
        for (uint64_t next = 0; next < n;) {
            uint64_t k = next + 1;  // (half >= the longest value: the first always fits)
            while (k < n && out_off[k + 1] - out_off[next] <= half) k++;
            Piece cur;
            cur.at = out_off[next];
            cur.len = out_off[k] - out_off[next];
            cur.buf = b;
            cur.live = cur.len != 0;
            if (cur.live) {
                uint8_t *piece = d_out.as<uint8_t>() + (size_t)b * half;
                if (ctl.n_desc)
                    AH_TRY(launch_write_descendants(src, g.out + next, k - next, g.len + next, g.info + next, cur.at, piece, any_bitmap, s));
                if (ctl.n_split) {
                    hipLaunchKernelGGL(k_ixenc_write_split, dim3(grid_of(k - next, kIxEncBlock / kWave, 256u * 16u)), dim3(kIxEncBlock), 0, s,
                                       g.out + next, g.info + next, k - next, g.len + next, cur.at, piece,
                                       reinterpret_cast<const uint32_t *>(ix->d_nrows), row_words32,
                                       reinterpret_cast<const uint32_t *>(ix->d_nhdrs), hf);
                    AH_HIP(hipGetLastError());
                }
                AH_HIP(hipMemcpyAsync(pin + (size_t)b * half, piece, (size_t)cur.len, hipMemcpyDeviceToHost, s));
                AH_HIP(hipEventRecord(ev[b], s));
                st.pieces++;
                b ^= 1;
            }
            // (the encode and the copy of this piece run while the host moves the one before out of its pinned half)
            if (cur.live && prev.live) AH_TRY(hand_over(prev));
            if (cur.live) prev = cur;
            next = k;
        }
        if (prev.live) AH_TRY(hand_over(prev));
    }
    st.seconds = IndexCall::secs(call.t0, IndexCall::now());
    if (out_stats) *out_stats = st;
    return AH_OK;
}

}  // namespace

extern "C" {

int ah_index_encode_nodes(ah_index *ix, const uint32_t *node_indices, size_t n, const uint32_t *node_id_of, uint32_t node_id_base,
                          uint8_t *out_values, uint64_t out_cap, uint64_t *out_value_offsets, ah_index_encode_stats *out_stats) {
    AH_GUARDED("ah_index_encode_nodes")
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_REQUIRE(out_value_offsets, AH_ERR_INVALID_ARGUMENT, "out_value_offsets is NULL");
    AH_INDEX_LIVE(ix);
    DeviceRestore restore_device;
    return encode_nodes_impl(ix, node_indices, n, node_id_of, node_id_base, out_values, out_cap, out_value_offsets, out_stats);
    AH_GUARDED_END
}

}  // extern "C"
