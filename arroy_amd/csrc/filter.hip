// filter.hip — resident candidate filters (`QueryBuilder::candidates` kept on the device of its index): everything that makes,
// edits, inspects or destroys one.  What a search reads of a filter is in filter.h (host) and filter_device.h (device); the block
// layout (FilterBlock), the counter layout (FilterCounter) and the creation path (FilterCall): DESIGN.md 4 "Filters: where things live".
#include <cassert>
#include <memory>
#include <optional>

#include "common.h"
#include "device_math.h"
#include "filter.h"
#include "roaring_parse.h"

namespace ah {

// What a filter call counts on the device, 64-bit words: the call's totals, then FC_PER_FILTER words per filter of the call.
enum FilterCounter { FC_REMOVED = 0, FC_ADDED, FC_LEAVES, FC_LEAVES_WALKED, FC_IDS_WALKED, FC_TOTALS, FC_LISTED = 0, FC_STORED, FC_PER_FILTER };
// One filter of a batched call, in device memory, indexed by the wave-uniform blockIdx.y (scalar loads): where its old bitmap is
// and how long (ah_filter_resume_batch), its new block, and its two edit lists as ranges of the call's one upload of ids.
struct CallFilter {
    const uint32_t *old_bits;
    uint64_t old_len_bits;
    uint32_t *bits;
    uint64_t remove_off, n_remove, add_off, n_add;
};
// How many of the listed ids are rows of the dataset, by its id -> row table (ah_filter_create on sparse ids; identity ids
// need no kernel: the ids below n).  One partial sum per wave.
__global__ __launch_bounds__(256) void k_filter_stored(DataView dv, const uint32_t *__restrict__ ids, uint64_t n,
                                                       unsigned long long *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t c = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) c += row_of_id(dv, ids[g]) != ~0ull ? 1u : 0u;
    for (uint32_t d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// ---- filter expressions (ah_filter_combine) ----------------------------------------------------------------------------
// The operands of one ah_filter_combine call, by value in the kernel arguments: their bitmaps (k_filter_combine) or their
// per-node arrays (k_leaf_kept_combine).  Indexed by a wave-uniform i < n only: scalar loads from the argument segment.
struct CombineTable {
    const uint32_t *p[AH_FILTER_COMBINE_MAX];
};

// Four words of operand 0 combined with the same four of the operands 1 .. n - 1.
template <int OP>
__device__ __forceinline__ uint4 combine_quad(const CombineTable &t, uint32_t n, uint64_t quad) {
    uint4 r = reinterpret_cast<const uint4 *>(t.p[0])[quad];
    for (uint32_t i = 1; i < n; i++) {
        const uint4 x = reinterpret_cast<const uint4 *>(t.p[i])[quad];
        if (OP == AH_FILTER_AND) r = make_uint4(r.x & x.x, r.y & x.y, r.z & x.z, r.w & x.w);
        else if (OP == AH_FILTER_OR) r = make_uint4(r.x | x.x, r.y | x.y, r.z | x.z, r.w | x.w);
        else r = make_uint4(r.x & ~x.x, r.y & ~x.y, r.z & ~x.z, r.w & ~x.w);  // AH_FILTER_ANDNOT
    }
    return r;
}
// The bits of word `w` of a bitmap of len_bits bits that lie below len_bits (the last word's tail and the padding words: 0).
__device__ __forceinline__ uint32_t word_mask(uint64_t w, uint64_t len_bits) {
    const uint64_t first = w << 5;
    if (first + 32 <= len_bits) return 0xFFFFFFFFu;
    if (first >= len_bits) return 0u;
    return (1u << (uint32_t)(len_bits - first)) - 1u;
}
template <int OP>
__device__ __forceinline__ unsigned long long combine_words(const CombineTable &t, uint32_t n, uint64_t n_quads, uint64_t len_bits,
                                                            uint32_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long set = 0;
    for (uint64_t quad = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; quad < n_quads; quad += stride) {
        uint4 r;
        if (OP == AH_FILTER_NOT) {  // the one op that can set a bit at or above len_bits
            const uint4 a = reinterpret_cast<const uint4 *>(t.p[0])[quad];
            r = make_uint4(~a.x & word_mask(4 * quad, len_bits), ~a.y & word_mask(4 * quad + 1, len_bits),
                           ~a.z & word_mask(4 * quad + 2, len_bits), ~a.w & word_mask(4 * quad + 3, len_bits));
        } else {
            r = combine_quad<OP>(t, n, quad);
        }
        reinterpret_cast<uint4 *>(out)[quad] = r;
        set += (uint32_t)(__popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w));
    }
    return set;
}
// The bitmap of an expression over resident filters: n_quads x 16 bytes (the blocks are 128-byte aligned, their word counts
// multiples of 64), every operand read once with 16-byte loads, and the number of set bits (which can pass 2^32: NOT of a small
// set where id u32::MAX is stored).  The operands keep "no bit at or above len_bits", so only NOT has to mask.
__global__ __launch_bounds__(256) void k_filter_combine(CombineTable t, uint32_t n, int op, uint64_t n_quads, uint64_t len_bits,
                                                        uint32_t *__restrict__ out, unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long s_part[4];
    unsigned long long set = 0;
    switch (op) {  // (uniform over the launch)
    case AH_FILTER_AND: set = combine_words<AH_FILTER_AND>(t, n, n_quads, len_bits, out); break;
    case AH_FILTER_OR: set = combine_words<AH_FILTER_OR>(t, n, n_quads, len_bits, out); break;
    case AH_FILTER_ANDNOT: set = combine_words<AH_FILTER_ANDNOT>(t, n, n_quads, len_bits, out); break;
    default: set = combine_words<AH_FILTER_NOT>(t, n, n_quads, len_bits, out); break;
    }
    block_add_u64(set, &counters[FC_TOTALS + FC_LISTED], s_part);
}

// How many rows of the dataset a bitmap over [0, len_bits) holds, by the dataset's ascending id array (sparse ids; with identity
// ids every set bit is a row): n loads, not a walk of a bitmap that may be 512 MiB.  Every id is below len_bits (the largest + 1).
// blockIdx.y names the filter: its bitmap is that of slots[blockIdx.y], or `bits` for the one filter of a call without a table
// (slots == nullptr, gridDim.y == 1); its sum goes to out[out_stride * blockIdx.y].
__global__ __launch_bounds__(256) void k_filter_stored_rows(const CallFilter *__restrict__ slots, const uint32_t *__restrict__ bits,
                                                            const uint32_t *__restrict__ ids, uint64_t n,
                                                            unsigned long long *__restrict__ out, uint32_t out_stride) {
    __shared__ unsigned long long s_part[4];
    if (slots) bits = slots[blockIdx.y].bits;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long c = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint32_t id = ids[g];
        c += (bits[id >> 5] >> (id & 31)) & 1u;
    }
    block_add_u64(c, out + (size_t)out_stride * blockIdx.y, s_part);
}

// |descendants & candidates| of every node under the NEW bitmap (lw.bits), one octet per node slot as k_leaf_kept.  With
// c the leaf's length and k_i what operand i keeps of it, the count follows from the k_i alone wherever all operands but at most
// one keep all or nothing of the leaf (`shortcut`; DESIGN.md 4 "Combined filters" has the rules and why they hold); only the
// other leaves are walked, with the arithmetic of copy_filtered.  A free slot, a split node or an empty leaf gives 0.
__global__ __launch_bounds__(256) void k_leaf_kept_combine(LeafWalk lw, uint32_t n_nodes, CombineTable kept_of, uint32_t n, int op,
                                                           int shortcut, uint32_t *__restrict__ kept,
                                                           unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long s_part[4];
    const uint32_t j = threadIdx.x & 7u;
    const uint32_t octets = (gridDim.x * blockDim.x) >> 3;
    uint32_t leaves = 0, walked = 0;  // (counted by lane 0 of the octet)
    unsigned long long ids_walked = 0;
    for (uint32_t node = (blockIdx.x * blockDim.x + threadIdx.x) >> 3; node < n_nodes; node += octets) {
        const DNode nd = lw.nodes[node];
        const uint32_t c = (nd.kind & 0xFFu) == AH_NODE_DESCENDANTS ? nd.b : 0u;
        uint32_t r = 0;
        bool walk = c != 0;
        if (c != 0 && shortcut) {
            const uint32_t k0 = kept_of.p[0][node];
            if (op == AH_FILTER_NOT) {
                r = c - k0;
                walk = false;
            } else if (op == AH_FILTER_ANDNOT) {  // k0 minus what the subtrahends take: nothing if they are all empty here
                bool any_full = false, all_zero = true;
                for (uint32_t i = 1; i < n; i++) {
                    const uint32_t k = kept_of.p[i][node];
                    any_full |= k == c;
                    all_zero &= k == 0;
                }
                if (k0 == 0 || any_full) r = 0, walk = false;
                else if (all_zero) r = k0, walk = false;
            } else {
                // AND: `settled` = an operand keeps nothing, `part` = operands that keep less than all, `ext` = the smallest count;
                // OR, the mirror image: an operand keeps all, operands that keep something, the largest count
                const bool is_and = op == AH_FILTER_AND;
                bool settled = false;
                uint32_t part = 0, ext = is_and ? c : 0u;
                for (uint32_t i = 0; i < n; i++) {
                    const uint32_t k = i ? kept_of.p[i][node] : k0;
                    settled |= k == (is_and ? 0u : c);
                    part += is_and ? (k < c) : (k > 0);
                    ext = is_and ? min(ext, k) : max(ext, k);
                }
                if (settled) r = is_and ? 0u : c, walk = false;
                else if (part <= 1) r = ext, walk = false;
            }
        }
        if (walk) r = copy_filtered(lw.bits, lw.len_bits, lw.desc + nd.a, c, nullptr, j);
        if (j == 0) {
            kept[node] = r;
            leaves += c != 0;
            walked += walk;
            ids_walked += walk ? c : 0u;
        }
    }
    block_add_u64(leaves, &counters[FC_LEAVES], s_part);
    block_add_u64(walked, &counters[FC_LEAVES_WALKED], s_part);
    block_add_u64(ids_walked, &counters[FC_IDS_WALKED], s_part);
}

// ---- filters across index maintenance (ah_filter_resume_batch) ----------------------------------------------------------
// 1. re-cut: the new block of every filter whole — the old words below min(old, new) len_bits (the last one masked), zero above
// (the padding words, the per-node counts k_leaf_kept_group writes afterwards, the tail).  Grid over (word, filter).
__global__ __launch_bounds__(256) void k_filter_recut(const CallFilter *__restrict__ slots, uint64_t len_bits, uint64_t words,
                                                      uint64_t block_words) {
    const CallFilter sl = slots[blockIdx.y];
    const uint64_t keep_bits = min(sl.old_len_bits, len_bits);  // (below it every word index is inside the old bitmap too)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t quad = first; quad < words / 4; quad += stride) {  // (words: a multiple of 64, the blocks 128-byte aligned)
        uint4 r = make_uint4(0, 0, 0, 0);
        if ((quad << 7) < keep_bits) {
            const uint4 a = reinterpret_cast<const uint4 *>(sl.old_bits)[quad];
            r = make_uint4(a.x & word_mask(4 * quad, keep_bits), a.y & word_mask(4 * quad + 1, keep_bits),
                           a.z & word_mask(4 * quad + 2, keep_bits), a.w & word_mask(4 * quad + 3, keep_bits));
        }
        reinterpret_cast<uint4 *>(sl.bits)[quad] = r;
    }
    for (uint64_t w = words + first; w < block_words; w += stride) sl.bits[w] = 0;
}

// 2. the host's delta: SET = false clears the bits of every filter's remove list, SET = true (the launch after it: an id in both
// lists ends up set) sets those of its add list.  Ids at or above len_bits match nothing and are skipped.  The lists are
// strictly ascending, so no two lanes flip the same bit and the number of bits that flipped is exact.
template <bool SET>
__global__ __launch_bounds__(256) void k_filter_edit(const CallFilter *__restrict__ slots, const uint32_t *__restrict__ ids,
                                                     uint64_t len_bits, unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long s_part[4];
    const CallFilter sl = slots[blockIdx.y];
    const uint32_t *list = ids + (SET ? sl.add_off : sl.remove_off);
    const uint64_t n = SET ? sl.n_add : sl.n_remove;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long flipped = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint32_t id = list[g];
        if (id >= len_bits) continue;
        const uint32_t bit = 1u << (id & 31);
        const uint32_t old = SET ? atomicOr(&sl.bits[id >> 5], bit) : atomicAnd(&sl.bits[id >> 5], ~bit);
        flipped += ((old & bit) != 0) != SET;
    }
    block_add_u64(flipped, &counters[SET ? FC_ADDED : FC_REMOVED], s_part);
}

// 3. `listed` of every filter: the set bits of its new bitmap; `stored` too on identity ids (sparse: k_filter_stored_rows per blockIdx.y)
__global__ __launch_bounds__(256) void k_filter_popcount(const CallFilter *__restrict__ slots, uint64_t words,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long s_part[4];
    const uint4 *bits = reinterpret_cast<const uint4 *>(slots[blockIdx.y].bits);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long set = 0;
    for (uint64_t quad = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; quad < words / 4; quad += stride) {
        const uint4 r = bits[quad];
        set += (uint32_t)(__popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w));
    }
    block_add_u64(set, &counters[FC_TOTALS + FC_PER_FILTER * blockIdx.y + FC_LISTED], s_part);
}

// 4. the per-node counts of up to AH_FILTER_RESUME_GROUP filters of one length in ONE pass over the Descendants ids.  The
// table travels in the kernel arguments and is indexed by unrolled constants only: the pointers are scalar loads.
struct CountGroup {
    uint32_t *block[AH_FILTER_RESUME_GROUP];  // FilterBlock: [bitmap: `words` words][the per-node counts]
};
// A gather of one word per id and filter is what a count pass costs (measured: DESIGN.md 4 "Filters across index maintenance"),
// and word w of 16 filters lies in 16 different cache lines.  So a group's bitmaps are first written side by side, word w of
// filter f at mixed[16 w + f]: the 16 words an id needs are then ONE 64-byte line.  One thread per word index, the 16 reads
// coalesced over the threads.  A short group is filled up with copies of its first filter (the host: ah_filter_resume_batch).
__global__ __launch_bounds__(256) void k_filter_interleave(CountGroup t, uint64_t used_words, uint4 *__restrict__ mixed) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < used_words; w += stride) {
#pragma unroll
        for (int q = 0; q < AH_FILTER_RESUME_GROUP / 4; q++)
            mixed[4 * w + q] = make_uint4(t.block[4 * q][w], t.block[4 * q + 1][w], t.block[4 * q + 2][w], t.block[4 * q + 3][w]);
    }
}
// One octet per node slot and 32 ids a step, as k_leaf_kept (copy_filtered): every id is loaded once and tested against the GN
// bitmaps into GN per-lane counters, summed over the octet at the end of the leaf.  The count of node slot `node` under filter f
// goes behind f's bitmap and is what k_leaf_kept writes: 0 for a free slot, a split node or an empty leaf.
//   <1, false>                       the bitmap of filter 0 itself: a pass per filter (AH_FILTER_RESUME_GROUP = 1, or bitmaps
//                                    too long to lay side by side)
//   <AH_FILTER_RESUME_GROUP, true>   `mixed` (k_filter_interleave): four 16-byte loads per id serve the whole group
// GN is a compile-time constant: the counters stay in registers.  Copies of a filter in the table have their counts written
// more than once, by the same lane.  count_leaves: this pass also counts the leaves (the first pass of a call); the ids are
// counted by every pass.
template <int GN, bool MIXED>
__global__ __launch_bounds__(256) void k_leaf_kept_group(const DNode *__restrict__ nodes, const uint32_t *__restrict__ desc,
                                                         uint32_t n_nodes, uint64_t len_bits, uint64_t words, CountGroup t,
                                                         const uint4 *__restrict__ mixed, int count_leaves,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long s_part[4];
    static_assert(MIXED ? GN == AH_FILTER_RESUME_GROUP : GN == 1, "see above");
    const uint32_t j = threadIdx.x & 7u;
    const uint32_t octets = (gridDim.x * blockDim.x) >> 3;
    uint32_t leaves = 0;  // (counted by lane 0 of the octet)
    unsigned long long ids_walked = 0;
    for (uint32_t node = (blockIdx.x * blockDim.x + threadIdx.x) >> 3; node < n_nodes; node += octets) {
        const DNode nd = nodes[node];
        const uint32_t c = (nd.kind & 0xFFu) == AH_NODE_DESCENDANTS ? nd.b : 0u;
        const uint32_t *ids = desc + nd.a;
        uint32_t cnt[GN];
#pragma unroll
        for (int f = 0; f < GN; f++) cnt[f] = 0;
        for (uint32_t base = 0; base < c; base += 32) {
            uint32_t word[4], shift[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t i = base + 8 * u + j;
                const uint32_t id = i < c ? ids[i] : 0u;
                in[u] = i < c && id < len_bits;
                word[u] = in[u] ? id >> 5 : 0u;  // (a lane past the leaf or the bitmap reads word 0 and counts nothing)
                shift[u] = id & 31u;
            }
            if (MIXED) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
#pragma unroll
                    for (int q = 0; q < GN / 4; q++) {
                        const uint4 x = mixed[4 * (uint64_t)word[u] + q];
                        cnt[4 * q] += in[u] ? (x.x >> shift[u]) & 1u : 0u;
                        cnt[4 * q + 1] += in[u] ? (x.y >> shift[u]) & 1u : 0u;
                        cnt[4 * q + 2] += in[u] ? (x.z >> shift[u]) & 1u : 0u;
                        cnt[4 * q + 3] += in[u] ? (x.w >> shift[u]) & 1u : 0u;
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) cnt[0] += in[u] ? (t.block[0][word[u]] >> shift[u]) & 1u : 0u;
            }
        }
#pragma unroll
        for (int f = 0; f < GN; f++) {
            uint32_t v = cnt[f];
            v += __shfl_xor(v, 1, 8);
            v += __shfl_xor(v, 2, 8);
            v += __shfl_xor(v, 4, 8);
            if (j == 0) t.block[f][words + node] = v;
        }
        if (j == 0) {
            leaves += c != 0;
            ids_walked += c;
        }
    }
    if (count_leaves) block_add_u64(leaves, &counters[FC_LEAVES], s_part);
    block_add_u64(ids_walked, &counters[FC_IDS_WALKED], s_part);
}

// ---- filters from serialized RoaringBitmaps (ah_filter_create_roaring_batch) --------------------------------------------------
// One travelling container of a call: whose it is, what the blob's headers say about it (roaring_parse.h), and where its payload
// lies in the call's staging buffer.  The host puts every payload at a 16-byte boundary and allots it whole 16-byte units, so a
// 16-byte load that begins inside a payload ends inside its allotment.
struct RoaringItem {
    uint32_t filter;       // the blob, and the slot of its filter in the call's CallFilter table
    uint32_t container;    // its position in the blob (for the error code)
    uint32_t key;          // id >> 16 of its span; at most (len_bits - 1) >> 16 (the host leaves the others behind)
    uint32_t kind;         // roaring::Kind
    uint32_t cardinality;  // 1 .. 65536; a KIND_ARRAY has at most 4096 (the kind follows from it)
    uint32_t n_runs;       // KIND_RUN: the runs behind the payload's first u16 (which the host has read)
    uint64_t payload;      // byte offset in the staging buffer, a multiple of 16
};
static_assert(sizeof(RoaringItem) == 32, "laid out by hand in the call's one upload");
// Why a payload was refused, in the low byte of the error code ((blob << 24) | (container << 8) | reason: the smallest code of a
// call is the one reported, hence the lowest (blob, container)).
enum RoaringReason : uint32_t { RR_ARRAY_ORDER = 1, RR_BITMAP_CARDINALITY, RR_RUN_ORDER, RR_RUN_PAST_END, RR_RUN_CARDINALITY };
constexpr uint32_t kRoaringSpanWords = 2048;  // the 32-bit words of a container's 64Ki ids

// One block per travelling container.  The container owns the 2048 words of its span in its filter's bitmap (the keys of a blob
// ascend strictly, every blob has its own filter), which the block writes with plain 16-byte stores over the zeroes of the
// call's memset: array and run containers through an 8 KiB image in LDS, bitmap containers straight through registers.  Nothing
// indexes by an unchecked value: array values and run bounds are 16 bits wide and address the image only, run ends are clamped
// to 65535 before use, and what leaves the block is masked against len_bits and never lies at or past the bitmap's used words.
// Counted: the bits written into `inside` of the filter (FC_LISTED of its counters; `stored` on identity ids), and all bits of
// the image against the cardinality the header states.  What fails a check goes into *err by one atomicMin.
__global__ __launch_bounds__(256) void k_roaring_expand(const RoaringItem *__restrict__ items, const uint8_t *__restrict__ staging,
                                                        const CallFilter *__restrict__ slots, uint64_t len_bits,
                                                        unsigned long long *__restrict__ counters, unsigned long long *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint32_t s_img[kRoaringSpanWords];
    __shared__ unsigned long long s_part[4];
    __shared__ uint32_t s_all[4], s_bad;
    const RoaringItem it = items[blockIdx.x];  // (wave-uniform: scalar loads)
    const uint32_t t = threadIdx.x;
    const uint8_t *payload = staging + it.payload;
    const uint4 *payload16 = reinterpret_cast<const uint4 *>(payload);
    const uint16_t *payload2 = reinterpret_cast<const uint16_t *>(payload);
    uint32_t *bits = slots[it.filter].bits;
    const uint64_t word0 = (uint64_t)it.key * kRoaringSpanWords, used_words = (len_bits + 31) >> 5;
    uint32_t bad = 0xFFFFFFFFu;  // the smallest reason this thread found
    if (t == 0) s_bad = 0xFFFFFFFFu;
    uint4 q[2];  // this thread's eight words of the span: quads t and t + 256
    if (it.kind == roaring::KIND_BITMAP) {
        q[0] = payload16[t];
        q[1] = payload16[t + 256];
        __syncthreads();  // (s_bad)
    } else {
        reinterpret_cast<uint4 *>(s_img)[t] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4 *>(s_img)[t + 256] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        if (it.kind == roaring::KIND_ARRAY) {
            // sixteen values a thread (two 16-byte loads); a value is compared with the one before it, the first of a thread with
            // the last of the thread before, read from the payload again
            const uint32_t first = 16 * t, card = min(it.cardinality, 4096u);
            uint32_t prev = first > 0 && first < card ? payload2[first - 1] : 0u;
            bool has_prev = first > 0;
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                if (first + 8 * h >= card) break;
                const uint4 x = payload16[2 * t + h];
                const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) {
                    if (first + 8 * h + k >= card) break;
                    const uint32_t v = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                    if (has_prev && v <= prev) bad = min(bad, (uint32_t)RR_ARRAY_ORDER);
                    atomicOr(&s_img[v >> 5], 1u << (v & 31));
                    prev = v;
                    has_prev = true;
                }
            }
        } else {
            // the runs dealt over the threads: edge words by atomic OR of masks, interior words whole (they are this run's alone
            // unless runs overlap, which is refused)
            for (uint32_t r = t; r < it.n_runs; r += 256) {
                const uint32_t start = payload2[1 + 2 * r];
                uint32_t end = start + payload2[2 + 2 * r];  // inclusive
                if (end > 0xFFFFu) {
                    bad = min(bad, (uint32_t)RR_RUN_PAST_END);
                    end = 0xFFFFu;
                }
                if (r > 0 && start <= (uint32_t)payload2[2 * r - 1] + (uint32_t)payload2[2 * r]) bad = min(bad, (uint32_t)RR_RUN_ORDER);
                const uint32_t fw = start >> 5, lw = end >> 5;
                const uint32_t head = 0xFFFFFFFFu << (start & 31), tail = 0xFFFFFFFFu >> (31 - (end & 31));
                if (fw == lw) {
                    atomicOr(&s_img[fw], head & tail);
                } else {
                    atomicOr(&s_img[fw], head);
                    for (uint32_t w = fw + 1; w < lw; w++) s_img[w] = 0xFFFFFFFFu;
                    atomicOr(&s_img[lw], tail);
                }
            }
        }
        __syncthreads();
        q[0] = reinterpret_cast<const uint4 *>(s_img)[t];
        q[1] = reinterpret_cast<const uint4 *>(s_img)[t + 256];
    }
    // the write-out: masked against len_bits, no word at or past the used words
    uint32_t all = 0;
    unsigned long long inside = 0;
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
        const uint64_t w = word0 + 4 * (uint64_t)(t + 256 * h);
        all += (uint32_t)(__popc(q[h].x) + __popc(q[h].y) + __popc(q[h].z) + __popc(q[h].w));
        if (w >= used_words) continue;
        const uint4 r = make_uint4(q[h].x & word_mask(w, len_bits), q[h].y & word_mask(w + 1, len_bits), q[h].z & word_mask(w + 2, len_bits),
                                   q[h].w & word_mask(w + 3, len_bits));
        inside += (uint32_t)(__popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w));
        if (w + 4 <= used_words) {
            *reinterpret_cast<uint4 *>(bits + w) = r;  // (the block is 128-byte aligned, w a multiple of 4)
        } else {
            bits[w] = r.x;
            if (w + 1 < used_words) bits[w + 1] = r.y;
            if (w + 2 < used_words) bits[w + 2] = r.z;
        }
    }
    block_add_u64(inside, &counters[FC_TOTALS + FC_PER_FILTER * it.filter + FC_LISTED], s_part);
    for (uint32_t d = 32; d > 0; d >>= 1) all += __shfl_xor(all, d, 64);
    if ((t & 63u) == 0) s_all[t >> 6] = all;
    if (bad != 0xFFFFFFFFu) atomicMin(&s_bad, bad);
    __syncthreads();
    if (t == 0) {
        uint32_t reason = s_bad;
        if (s_all[0] + s_all[1] + s_all[2] + s_all[3] != it.cardinality)
            reason = min(reason, (uint32_t)(it.kind == roaring::KIND_BITMAP ? RR_BITMAP_CARDINALITY
                                             : it.kind == roaring::KIND_RUN  ? RR_RUN_CARDINALITY
                                                                              : RR_ARRAY_ORDER));  // (an array: a value twice)
        if (reason != 0xFFFFFFFFu)
            atomicMin(err, ((unsigned long long)it.filter << 24) | ((unsigned long long)it.container << 8) | reason);
    }
}

// ---- exhausted filters: kept_total and the kept list K(f) of a resident filter (DESIGN.md 4 "Exhausted filters") ----------
// kept_total(f): the sum of the per-node counts (k_leaf_kept), grid-stride.
__global__ __launch_bounds__(256) void k_kept_total(const uint32_t *__restrict__ leaf_kept, uint32_t n_nodes, unsigned long long *total) {
    __shared__ unsigned long long s_part[4];
    unsigned long long v = 0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += step) v += leaf_kept[i];
    block_add_u64(v, total, s_part);
}
// The ids the filter keeps of EVERY in-use leaf, as bits of `mark` (zeroed, over [0, filter_len_bits)): one octet per node slot,
// the launch shape of k_leaf_kept.  A node whose count is 0 (free slot, split node, leaf the filter keeps nothing of) is
// skipped; the ids of the others are tested as copy_filtered tests them.  walked: the leaves whose ids were tested.
__global__ __launch_bounds__(256) void k_kept_mark(LeafWalk lw, uint32_t n_nodes, const uint32_t *__restrict__ leaf_kept,
                                                   uint32_t *__restrict__ mark, unsigned long long *walked) {
    __shared__ unsigned long long s_part[4];
    const uint32_t j = threadIdx.x & 7u;
    const uint32_t octets = (gridDim.x * blockDim.x) >> 3;
    unsigned long long mine = 0;
    for (uint32_t node = (blockIdx.x * blockDim.x + threadIdx.x) >> 3; node < n_nodes; node += octets) {
        if (leaf_kept[node] == 0) continue;
        const DNode nd = lw.nodes[node];
        if ((nd.kind & 0xFFu) != AH_NODE_DESCENDANTS) continue;
        const uint32_t *ids = lw.desc + nd.a;
        for (uint32_t i = j; i < nd.b; i += 8) {
            const uint32_t id = ids[i];
            if (id < lw.len_bits && ((lw.bits[id >> 5] >> (id & 31)) & 1u)) atomicOr(&mark[id >> 5], 1u << (id & 31));
        }
        if (j == 0) mine++;
    }
    block_add_u64(mine, walked, s_part);
}
// The set bits of a bitmap as an ascending id list, kBitmapListWords words a block: k_bitmap_count leaves every block's
// popcount, launch_scan_sums makes them offsets, k_bitmap_list counts again and writes the ids behind its block's offset.
// block0: the first block of this launch (the passes run in spans of AH_LAUNCH_MAX_ITEMS words).
static constexpr uint32_t kBitmapListWords = 2048;  // 256 threads x 8 words
__global__ __launch_bounds__(256) void k_bitmap_count(const uint32_t *__restrict__ bits, uint64_t words, uint32_t block0,
                                                      uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_wave[4];
    const uint32_t block = block0 + blockIdx.x;
    const uint64_t base = (uint64_t)block * kBitmapListWords + (uint64_t)threadIdx.x * 8;
    uint32_t c = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) c += base + e < words ? (uint32_t)__popc(bits[base + e]) : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) sums[block] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}
__global__ __launch_bounds__(256) void k_bitmap_list(const uint32_t *__restrict__ bits, uint64_t words, uint32_t block0,
                                                     const uint32_t *__restrict__ offsets, uint64_t n, uint32_t *__restrict__ out) {
    __shared__ uint32_t s_wave[4];
    const uint32_t block = block0 + blockIdx.x;
    const uint64_t base = (uint64_t)block * kBitmapListWords + (uint64_t)threadIdx.x * 8;
    uint32_t w[8], local = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        w[e] = base + e < words ? bits[base + e] : 0u;
        local += (uint32_t)__popc(w[e]);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if ((int)lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint64_t pos = (uint64_t)offsets[block] + incl - local;
    for (uint32_t v = 0; v < wave; v++) pos += s_wave[v];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        uint32_t left = w[e];
        while (left) {
            const uint32_t bit = (uint32_t)__ffs((int)left) - 1u;
            if (pos < n) out[pos] = (uint32_t)((base + e) << 5) + bit;  // (pos < n: the bitmap is the one that was counted)
            pos++;
            left &= left - 1u;
        }
    }
}

// The block of a filter of `ix`: [bitmap: `words` 32-bit words, a multiple of 64, zero from len_bits on][n_nodes per-node
// counts][256 bytes].  A call that makes one filter counts on the device into the first 8-byte aligned words of that tail
// (FilterCounter with one filter), which no search reads.
struct FilterBlock {
    uint64_t len_bits;
    size_t words, counters_off, bytes;
    FilterBlock(const ah_index *ix, uint64_t bits) : len_bits(bits) {
        words = (((size_t)len_bits + 31) / 32 + 63) & ~(size_t)63;
        counters_off = (words * 4 + (size_t)ix->n_nodes * 4 + 7) & ~(size_t)7;
        bytes = words * 4 + (size_t)ix->n_nodes * 4 + 256;
        static_assert((FC_TOTALS + FC_PER_FILTER) * 8 + 8 <= 256, "the counters live in the block's tail");
    }
};
// How a call that makes the per-node counts of many filters of one length groups them (ah_filter_resume_batch,
// ah_filter_create_roaring_batch).  A group's bitmaps side by side (k_filter_interleave) take 64 bytes per bitmap word: where that
// passes the budget (256 MiB: ids beyond 2^27) the counts are made a filter a pass, as ah_filter_create makes them.
struct GroupPlan {
    uint64_t used_words;
    size_t mixed_bytes, group;
    explicit GroupPlan(const FilterBlock &fb) : used_words((fb.len_bits + 31) / 32) {
        mixed_bytes = std::max<size_t>(1, (size_t)used_words) * AH_FILTER_RESUME_GROUP * 4;
        group = (size_t)std::min<long long>(AH_FILTER_RESUME_GROUP, std::max<long long>(1, tun(TUN_FILTER_RESUME_GROUP)));
        if (mixed_bytes > ((size_t)std::max<long long>(0, tun(TUN_FILTER_RESUME_MIXED_MB)) << 20)) group = 1;
    }
    size_t groups_of(size_t n) const { return (n + group - 1) / group; }
};
// The per-node counts of the filters in `blocks` (FilterBlock layout, bitmaps finished on the stream), a group a pass;
// `mixed`: gp.mixed_bytes where gp.group > 1.  FC_LEAVES and FC_IDS_WALKED of `d_counters` are counted.
static void launch_leaf_kept_groups(const ah_index *ix, const FilterBlock &fb, const GroupPlan &gp, const std::vector<DevMem> &blocks,
                                    const DevMem &mixed, unsigned long long *d_counters, hipStream_t s) {
    const uint32_t n_nodes = ix->n_nodes;
    const size_t n = blocks.size();
    if (!n_nodes) return;
    for (size_t g0 = 0; g0 < n; g0 += gp.group) {
        const size_t g = std::min(gp.group, n - g0);
        CountGroup t{};
        for (size_t f = 0; f < AH_FILTER_RESUME_GROUP; f++) t.block[f] = blocks[g0 + (f < g ? f : 0)].as<uint32_t>();
        const dim3 grid(grid_of(n_nodes, 32, 2048));
        if (gp.group == 1 || g == 1) {  // (a group of one reads its own bitmap: nothing to lay side by side)
            hipLaunchKernelGGL((k_leaf_kept_group<1, false>), grid, dim3(256), 0, s, ix->d_nodes, ix->d_desc, n_nodes, fb.len_bits,
                               (uint64_t)fb.words, t, (const uint4 *)nullptr, g0 == 0 ? 1 : 0, d_counters);
            continue;
        }
        // (one stream: the pass before has read `mixed` before this group's words are written over it)
        if (gp.used_words)
            hipLaunchKernelGGL(k_filter_interleave, dim3(grid_of(gp.used_words, 256, 2048)), dim3(256), 0, s, t, gp.used_words, mixed.as<uint4>());
        hipLaunchKernelGGL((k_leaf_kept_group<AH_FILTER_RESUME_GROUP, true>), grid, dim3(256), 0, s, ix->d_nodes, ix->d_desc, n_nodes,
                           fb.len_bits, (uint64_t)fb.words, t, mixed.as<const uint4>(), g0 == 0 ? 1 : 0, d_counters);
    }
}

// A finished filter joins its index: the counters of ah_filter_stats move, the block is the filter's from here.  `passes`: what
// its per-node counts cost in passes over the Descendants ids (a batched call charges its groups to its first filter).
static void filter_adopt(ah_filter *f, ah_index *ix, DevMem &block, const FilterBlock &fb, uint64_t listed, uint64_t stored,
                         uint64_t passes) {
    f->listed = listed;
    f->stored = stored;
    f->d_bits = block.as<uint32_t>();
    f->d_leaf_kept = f->d_bits + fb.words;
    f->device_bytes = dev_block_bytes(block.p);  // (what the allocator accounts for it: ah_device_cache_stats)
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->fstats.filters_created++;
        ix->fstats.filters_alive++;
        ix->fstats.leaf_kept_passes += ix->n_nodes ? passes : 0;
    }
    block.p = nullptr;
}
static int filter_index_live(const ah_index *ix) {
    AH_REQUIRE(ix && ix->ds, AH_ERR_INVALID_ARGUMENT, "index is NULL");
    AH_INDEX_LIVE(ix);
    return AH_OK;
}
// The creation path, what the four creators do around their own bitmap step on n filters of one index: begin() (the device, the
// n handles, the n blocks of one FilterBlock), the call's other allocations, stream() (the leased context), the bitmap step and
// the count kernels, finish() (the launches' status, the counters read back, the call's ONE synchronisation), adopt() per filter
// — never before finish() has returned AH_OK; a failure frees everything.  ah_filter_resume_batch keeps its handles (begin with
// handles = false) and has a hand-over of its own.
struct FilterCall {
    ah_index *ix;
    ah_dataset *ds;
    const FilterBlock fb;
    std::vector<std::unique_ptr<ah_filter>> fs;
    std::vector<DevMem> blocks;
    std::optional<ContextLease> lease;
    hipStream_t s = nullptr;
    explicit FilterCall(ah_index *ix) : ix(ix), ds(ix->ds), fb(ix, filter_len_bits(ix->ds)) {}

    int begin(size_t n, bool handles = true) {
        AH_HIP(hipSetDevice(ds->device));
        fs.resize(handles ? n : 0);
        for (auto &f : fs) {
            f.reset(new ah_filter);
            f->ix = ix;
            f->len_bits = fb.len_bits;
        }
        blocks = std::vector<DevMem>(n);
        for (DevMem &b : blocks) AH_HIP(dev_malloc(&b.p, fb.bytes));
        return AH_OK;
    }
    int stream() {
        lease.emplace(ds);
        AH_REQUIRE(lease->c, AH_ERR_DEVICE, "cannot create a HIP stream");
        s = lease->c->stream;
        return AH_OK;
    }
    uint32_t *bits() const { return blocks[0].as<uint32_t>(); }  // of a call that makes one filter, as kept() and counters()
    uint32_t *kept() const { return bits() + fb.words; }
    unsigned long long *counters() const { return reinterpret_cast<unsigned long long *>(blocks[0].as<uint8_t>() + fb.counters_off); }
    void leaf_kept() const {  // the per-node counts of the one filter's bitmap as it is on the stream
        if (ix->n_nodes) launch_leaf_kept(ix, bits(), fb.len_bits, kept(), s);
    }
    void stored_rows() const {  // `stored` of the one filter on sparse ids, likewise
        hipLaunchKernelGGL(k_filter_stored_rows, dim3((uint32_t)std::min<uint64_t>((ds->n + 255) / 256, 2048)), dim3(256), 0, s,
                           (const CallFilter *)nullptr, (const uint32_t *)bits(), ds->view().ids, (uint64_t)ds->n,
                           counters() + FC_TOTALS + FC_STORED, 0u);
    }
    int finish(unsigned long long *h, const unsigned long long *d_counters, size_t words) {
        AH_HIP(hipGetLastError());
        if (words) AH_HIP(hipMemcpyAsync(h, d_counters, words * 8, hipMemcpyDeviceToHost, s));
        AH_HIP(hipStreamSynchronize(s));
        return AH_OK;
    }
    void adopt(size_t i, uint64_t listed, uint64_t stored, uint64_t passes, ah_filter **out) {
        filter_adopt(fs[i].get(), ix, blocks[i], fb, listed, stored, passes);
        *out = fs[i].release();
    }
};
// kept_total(f), made on `ctx` the first time (one reduction over the per-node counts).
int filter_kept_total(ah_filter *f, Context *ctx, uint64_t &out) {
    if (!f->total_ready.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lk(f->list_mu);
        if (!f->total_ready.load(std::memory_order_relaxed)) {
            const ah_index *ix = f->ix;
            unsigned long long total = 0;
            if (ix->n_nodes) {
                AH_TRY(ctx->ensure_device(256));
                unsigned long long *d_total = reinterpret_cast<unsigned long long *>(ctx->d_scratch);
                AH_HIP(hipMemsetAsync(d_total, 0, 8, ctx->stream));
                hipLaunchKernelGGL(k_kept_total, dim3(grid_of(ix->n_nodes, 1024, 1024)), dim3(256), 0, ctx->stream, f->d_leaf_kept, ix->n_nodes,
                                   d_total);
                AH_HIP(hipGetLastError());
                AH_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
                AH_HIP(hipStreamSynchronize(ctx->stream));
            }
            f->kept_total = total;
            f->total_ready.store(true, std::memory_order_release);
        }
    }
    out = f->kept_total;
    return AH_OK;
}

// K(f), made on `ctx` the first time: k_kept_mark into a transient bitmap, then its set bits as a list (k_bitmap_count,
// launch_scan_sums, k_bitmap_list).  Nothing of a failed attempt stays: the next request starts again.
int filter_kept_list(ah_filter *f, Context *ctx) {
    if (f->list_ready.load(std::memory_order_acquire)) return AH_OK;
    std::lock_guard<std::mutex> lk(f->list_mu);
    if (f->list_ready.load(std::memory_order_relaxed)) return AH_OK;
    ah_index *ix = f->ix;
    hipStream_t s = ctx->stream;
    const uint64_t words = (f->len_bits + 31) / 32;
    unsigned long long walked = 0;
    uint32_t n = 0;
    DevMem list;
    if (words && ix->n_nodes) {
        const uint32_t n_blocks = (uint32_t)((words + kBitmapListWords - 1) / kBitmapListWords);
        // [mark: words][block sums: n_blocks][the total][pad to 8][leaves walked: 8 bytes]
        const size_t sums_off = (size_t)words * 4, total_off = sums_off + (size_t)n_blocks * 4, walked_off = (total_off + 4 + 7) & ~(size_t)7;
        DevMem work;
        AH_TRY(alloc(&work, walked_off + 8, "the kept list of a filter"));
        uint32_t *d_mark = work.as<uint32_t>(), *d_sums = reinterpret_cast<uint32_t *>(work.as<uint8_t>() + sums_off);
        uint32_t *d_n = reinterpret_cast<uint32_t *>(work.as<uint8_t>() + total_off);
        unsigned long long *d_walked = reinterpret_cast<unsigned long long *>(work.as<uint8_t>() + walked_off);
        AH_HIP(hipMemsetAsync(work.p, 0, walked_off + 8, s));
        launch_leaf_walk(k_kept_mark, dim3(1024), ix, f->d_bits, f->len_bits, s, (const uint32_t *)f->d_leaf_kept, d_mark, d_walked);
        const uint32_t span = (uint32_t)std::max<long long>(1, std::min<long long>(tun(TUN_LAUNCH_MAX_ITEMS), 0xFFFFFFFFll) / kBitmapListWords);
        for (uint32_t b0 = 0; b0 < n_blocks; b0 += span)
            hipLaunchKernelGGL(k_bitmap_count, dim3(std::min(span, n_blocks - b0)), dim3(256), 0, s, d_mark, words, b0, d_sums);
        AH_HIP(hipGetLastError());
        AH_TRY(launch_scan_sums(d_sums, n_blocks, d_n, s));
        AH_HIP(hipMemcpyAsync(&n, d_n, 4, hipMemcpyDeviceToHost, s));
        AH_HIP(hipMemcpyAsync(&walked, d_walked, 8, hipMemcpyDeviceToHost, s));
        AH_HIP(hipStreamSynchronize(s));
        if (n) {
            AH_TRY(alloc(&list, (size_t)n * 4, "the kept list of a filter"));
            for (uint32_t b0 = 0; b0 < n_blocks; b0 += span)
                hipLaunchKernelGGL(k_bitmap_list, dim3(std::min(span, n_blocks - b0)), dim3(256), 0, s, d_mark, words, b0, d_sums, (uint64_t)n,
                                   list.as<uint32_t>());
            AH_HIP(hipGetLastError());
            AH_HIP(hipStreamSynchronize(s));
        }
    }
    f->n_list = n;
    f->d_list = list.as<uint32_t>();
    f->list_bytes = n ? dev_block_bytes(list.p) : 0;
    f->device_bytes.fetch_add(f->list_bytes, std::memory_order_relaxed);
    list.p = nullptr;  // the filter owns it from here
    {
        std::lock_guard<std::mutex> sl(ix->stats_mu);
        ix->xstats.lists_made += n ? 1 : 0;
        ix->xstats.list_ids += n;
        ix->xstats.leaves_walked += walked;
    }
    f->list_ready.store(true, std::memory_order_release);
    return AH_OK;
}
// ah_filter_suspend / ah_filter_destroy: the list goes, and with it what was derived from the per-node counts
static void filter_drop_list(ah_filter *f) {
    std::lock_guard<std::mutex> lk(f->list_mu);
    if (f->d_list) (void)dev_free(f->d_list);
    f->device_bytes.fetch_sub(f->list_bytes, std::memory_order_relaxed);
    f->d_list = nullptr;
    f->n_list = f->list_bytes = f->kept_total = 0;
    f->list_ready.store(false, std::memory_order_release);
    f->total_ready.store(false, std::memory_order_release);
}

}  // namespace ah

using namespace ah;

extern "C" {

// ---- resident candidate filters (include/arroy_hip.h) ---------------------------------------------------------------------

int ah_filter_create(ah_index *ix, const uint32_t *sorted_ids, size_t n, ah_filter **out) {
    AH_GUARDED("ah_filter_create")
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    AH_REQUIRE(n == 0 || sorted_ids, AH_ERR_INVALID_ARGUMENT, "sorted_ids is NULL");
    for (size_t i = 1; i < n; i++)
        AH_REQUIRE(sorted_ids[i - 1] < sorted_ids[i], AH_ERR_INVALID_ARGUMENT, "sorted_ids is not strictly ascending at position %zu (%u after %u)",
                   i, sorted_ids[i], sorted_ids[i - 1]);
    AH_TRY(filter_index_live(ix));
    FilterCall call(ix);
    AH_TRY(call.begin(1));
    // bitmap over item ids (ids beyond the largest stored id cannot match: the list is ascending), then one word per node
    const size_t n_keep = filter_list_cut(sorted_ids, n, call.fb.len_bits);
    DevMem list;  // (the ids that travel, gone when this call returns)
    if (n_keep) AH_HIP(dev_malloc(&list.p, n_keep * 4));
    AH_TRY(call.stream());
    hipStream_t s = call.s;
    AH_HIP(hipMemsetAsync(call.bits(), 0, call.fb.bytes, s));
    unsigned long long stored = n_keep;  // identity ids: every id up to n - 1 is a row; sparse ids: n_keep look-ups
    const bool count_on_device = n_keep && !call.ds->identity_ids;
    unsigned long long *d_stored = call.counters() + FC_TOTALS + FC_STORED;
    if (n_keep) {
        AH_HIP(hipMemcpyAsync(list.p, sorted_ids, n_keep * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_filter_bitmap, dim3(256), dim3(256), 0, s, list.as<const uint32_t>(), (uint64_t)n_keep, call.bits());
        if (count_on_device)
            hipLaunchKernelGGL(k_filter_stored, dim3(256), dim3(256), 0, s, call.ds->view(), list.as<const uint32_t>(), (uint64_t)n_keep, d_stored);
    }
    call.leaf_kept();
    AH_TRY(call.finish(&stored, d_stored, count_on_device ? 1 : 0));
    call.adopt(0, n, stored, 1, out);
    return AH_OK;
    AH_GUARDED_END
}

// An expression over resident filters as a new resident filter (include/arroy_hip.h): one streaming pass over the operands'
// bitmaps, `stored` from the popcount (identity ids) or the dataset's id array, the per-node counts derived from the operands'
// wherever they settle it.  Works on the calling thread's leased context; one synchronisation, at the end.
int ah_filter_combine(int op, ah_filter *const *operands, size_t n, ah_filter **out, ah_filter_combine_stats *out_stats) {
    AH_GUARDED("ah_filter_combine")
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    AH_REQUIRE(op >= AH_FILTER_AND && op <= AH_FILTER_NOT, AH_ERR_INVALID_ARGUMENT, "unknown op %d (AH_FILTER_AND = 0 .. AH_FILTER_NOT = 3)", op);
    AH_REQUIRE(n >= 1 && n <= AH_FILTER_COMBINE_MAX, AH_ERR_INVALID_ARGUMENT, "n = %zu operands: 1 .. %d are legal", n,
               AH_FILTER_COMBINE_MAX);
    AH_REQUIRE(op != AH_FILTER_NOT || n == 1, AH_ERR_INVALID_ARGUMENT, "AH_FILTER_NOT takes exactly one operand (n = %zu)", n);
    AH_REQUIRE(operands, AH_ERR_INVALID_ARGUMENT, "operands is NULL");
    for (size_t i = 0; i < n; i++) AH_REQUIRE(operands[i], AH_ERR_INVALID_ARGUMENT, "operands[%zu] is NULL", i);
    ah_index *ix = operands[0]->ix;
    for (size_t i = 1; i < n; i++)
        AH_REQUIRE(operands[i]->ix == ix, AH_ERR_INVALID_ARGUMENT, "operands[%zu] belongs to another index than operands[0]", i);
    AH_TRY(filter_index_live(ix));
    for (size_t i = 0; i < n; i++)
        AH_REQUIRE(!operands[i]->suspended, AH_ERR_INVALID_ARGUMENT, "operands[%zu] is suspended (ah_filter_suspend): ah_filter_resume_batch it first", i);
    FilterCall call(ix);
    const FilterBlock &fb = call.fb;
    // (all filters of an index have one length: a dataset cannot change under a live index)
    for (size_t i = 0; i < n; i++) assert(operands[i]->len_bits == fb.len_bits);
    AH_TRY(call.begin(1));
    AH_TRY(call.stream());
    hipStream_t s = call.s;
    unsigned long long *d_counters = call.counters();
    // (the kernels write every bitmap word and every node's count; what they leave is the tail with the counters)
    AH_HIP(hipMemsetAsync(call.kept() + ix->n_nodes, 0, 256, s));
    CombineTable bits_of{}, kept_of{};
    for (size_t i = 0; i < n; i++) {
        bits_of.p[i] = operands[i]->d_bits;
        kept_of.p[i] = operands[i]->d_leaf_kept;
    }
    const uint64_t n_quads = fb.words / 4;
    if (n_quads)
        hipLaunchKernelGGL(k_filter_combine, dim3((uint32_t)std::min<uint64_t>((n_quads + 255) / 256, 2048)), dim3(256), 0, s, bits_of,
                           (uint32_t)n, op, n_quads, fb.len_bits, call.bits(), d_counters);
    const bool count_rows = !call.ds->identity_ids && call.ds->n;  // identity ids: every set bit is a row
    if (count_rows) call.stored_rows();
    if (ix->n_nodes)
        launch_leaf_walk(k_leaf_kept_combine, dim3((uint32_t)std::min<uint64_t>(((uint64_t)ix->n_nodes + 31) / 32, 1024)), ix, call.bits(),
                         fb.len_bits, s, kept_of, (uint32_t)n, op, tun(TUN_FILTER_COMBINE_SHORTCUT) != 0 ? 1 : 0, call.kept(), d_counters);
    unsigned long long h[FC_TOTALS + FC_PER_FILTER] = {};
    AH_TRY(call.finish(h, d_counters, FC_TOTALS + FC_PER_FILTER));
    if (out_stats) *out_stats = ah_filter_combine_stats{fb.words, h[FC_LEAVES], h[FC_LEAVES_WALKED], h[FC_IDS_WALKED]};
    call.adopt(0, h[FC_TOTALS + FC_LISTED], h[FC_TOTALS + (count_rows ? FC_STORED : FC_LISTED)], 1, out);
    return AH_OK;
    AH_GUARDED_END
}

// A filter from the host's own bitmap (include/arroy_hip.h): the bits up to the largest stored id travel as they are, `stored`
// and the per-node counts as ah_filter_combine / ah_filter_create make them.
int ah_filter_create_bitmap(ah_index *ix, const uint64_t *words, uint64_t n_bits, ah_filter **out) {
    AH_GUARDED("ah_filter_create_bitmap")
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    AH_REQUIRE(n_bits == 0 || words, AH_ERR_INVALID_ARGUMENT, "words is NULL");
    AH_TRY(filter_index_live(ix));
    FilterCall call(ix);
    // the set bits among the first `upto`
    auto popcount_below = [&](uint64_t upto) {
        uint64_t c = 0;
        for (uint64_t w = 0; w < (upto >> 6); w++) c += (uint64_t)__builtin_popcountll(words[w]);
        if (upto & 63) c += (uint64_t)__builtin_popcountll(words[upto >> 6] & ((1ull << (upto & 63)) - 1));
        return c;
    };
    const uint64_t n_travel = std::min(n_bits, call.fb.len_bits);  // bits above the largest stored id match nothing: they stay behind
    const uint64_t inside = popcount_below(n_travel);
    const uint64_t listed = n_travel == n_bits ? inside : popcount_below(n_bits);
    AH_TRY(call.begin(1));
    AH_TRY(call.stream());
    hipStream_t s = call.s;
    uint32_t *d_bits = call.bits();
    AH_HIP(hipMemsetAsync(d_bits, 0, call.fb.bytes, s));
    // whole 32-bit words as they are (little-endian: bit i of the 64-bit layout is bit i of the 32-bit one), the last one masked
    const size_t whole = (size_t)(n_travel >> 5);
    uint32_t last = 0;
    if (whole) AH_HIP(hipMemcpyAsync(d_bits, words, whole * 4, hipMemcpyHostToDevice, s));
    if (n_travel & 31) {
        memcpy(&last, reinterpret_cast<const uint8_t *>(words) + whole * 4, 4);
        last &= (1u << (uint32_t)(n_travel & 31)) - 1u;
        AH_HIP(hipMemcpyAsync(d_bits + whole, &last, 4, hipMemcpyHostToDevice, s));
    }
    const bool count_rows = !call.ds->identity_ids && call.ds->n && inside;  // identity ids: every bit below len_bits = n is a row
    if (count_rows) call.stored_rows();
    call.leaf_kept();
    unsigned long long stored = inside;
    AH_TRY(call.finish(&stored, call.counters() + FC_TOTALS + FC_STORED, count_rows ? 1 : 0));
    call.adopt(0, listed, stored, 1, out);
    return AH_OK;
    AH_GUARDED_END
}

// Test aid: the filter as it is on the device.  Reads only.
int ah_filter_export(const ah_filter *f, uint64_t *out_len_bits, uint32_t *out_bits, uint32_t *out_leaf_kept) {
    AH_GUARDED("ah_filter_export")
    AH_REQUIRE(f && f->ix && f->ix->ds, AH_ERR_INVALID_ARGUMENT, "filter is NULL");
    AH_REQUIRE(!f->suspended, AH_ERR_INVALID_ARGUMENT, "the filter is suspended (ah_filter_suspend): ah_filter_resume_batch it first");
    if (out_len_bits) *out_len_bits = f->len_bits;
    const ah_index *ix = f->ix;
    AH_HIP(hipSetDevice(ix->ds->device));
    ContextLease lease(ix->ds);
    AH_REQUIRE(lease.c, AH_ERR_DEVICE, "cannot create a HIP stream");
    hipStream_t s = lease.c->stream;
    const size_t words = ((size_t)f->len_bits + 31) / 32;
    if (out_bits && words) AH_HIP(hipMemcpyAsync(out_bits, f->d_bits, words * 4, hipMemcpyDeviceToHost, s));
    if (out_leaf_kept && ix->n_nodes) AH_HIP(hipMemcpyAsync(out_leaf_kept, f->d_leaf_kept, (size_t)ix->n_nodes * 4, hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    return AH_OK;
    AH_GUARDED_END
}

int ah_filter_info(const ah_filter *f, uint64_t *out_listed, uint64_t *out_stored, uint64_t *out_device_bytes) {
    AH_GUARDED("ah_filter_info")
    AH_REQUIRE(f, AH_ERR_INVALID_ARGUMENT, "filter is NULL");
    if (out_listed) *out_listed = f->listed;
    if (out_stored) *out_stored = f->stored;
    if (out_device_bytes) *out_device_bytes = f->device_bytes;
    return AH_OK;
    AH_GUARDED_END
}

int ah_filter_destroy(ah_filter *f) {
    AH_GUARDED("ah_filter_destroy")
    if (!f) return AH_OK;
    NoFailScope no_fail;
    ah_index *ix = f->ix;
    if (ix && ix->ds) (void)hipSetDevice(ix->ds->device);
    filter_drop_list(f);
    if (f->d_bits) (void)dev_free(f->d_bits);  // (waits for the device: no queued search still reads it)
    if (ix) {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        uint64_t &level = f->suspended ? ix->filters_suspended : ix->fstats.filters_alive;
        if (level) level--;
    }
    delete f;
    return AH_OK;
    AH_GUARDED_END
}

// ---- filters across index maintenance (include/arroy_hip.h) ---------------------------------------------------------------

int ah_filter_suspend(ah_filter *f) {
    AH_GUARDED("ah_filter_suspend")
    AH_REQUIRE(f && f->ix && f->ix->ds, AH_ERR_INVALID_ARGUMENT, "filter is NULL");
    AH_REQUIRE(!f->suspended, AH_ERR_INVALID_ARGUMENT, "the filter is suspended already");
    ah_index *ix = f->ix;
    AH_INDEX_LIVE(ix);
    {
        // no queued search reads the per-node counts any more (ah_index_suspend, for the rows)
        DeviceRestore restore_device;
        AH_HIP(hipSetDevice(ix->ds->device));
        AH_HIP(hipDeviceSynchronize());
        NoFailScope no_fail;
        filter_drop_list(f);  // (made from the per-node counts, which go stale: remade on first use after the resume)
    }
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    f->suspended = true;
    if (ix->fstats.filters_alive) ix->fstats.filters_alive--;
    ix->filters_suspended++;
    return AH_OK;
    AH_GUARDED_END
}

int ah_index_filters_suspended(ah_index *ix, uint64_t *out) {
    AH_GUARDED("ah_index_filters_suspended")
    AH_REQUIRE(ix && out, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    *out = ix->filters_suspended;
    return AH_OK;
    AH_GUARDED_END
}

// Suspended filters back on their index as it is now (include/arroy_hip.h).  Everything is queued on the calling thread's leased
// context — re-cut, clears, sets, `listed` / `stored`, then one k_leaf_kept_group per group — with one synchronisation at the
// end; the filters change hands only after it, where nothing can fail any more.
int ah_filter_resume_batch(ah_filter *const *filters, const ah_filter_edit *edits, size_t n, ah_filter_resume_stats *out_stats) {
    AH_GUARDED("ah_filter_resume_batch")
    if (out_stats) *out_stats = ah_filter_resume_stats{};
    if (n == 0) return AH_OK;
    // (what can be judged without a filter first)
    AH_REQUIRE(filters, AH_ERR_INVALID_ARGUMENT, "filters is NULL");
    AH_REQUIRE(n < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT, "too many filters");
    uint64_t n_edit_ids = 0;
    if (edits)
        for (size_t i = 0; i < n; i++) {
            const ah_filter_edit &e = edits[i];
            AH_REQUIRE(e.n_remove == 0 || e.remove_sorted, AH_ERR_INVALID_ARGUMENT, "edits[%zu].remove_sorted is NULL", i);
            AH_REQUIRE(e.n_add == 0 || e.add_sorted, AH_ERR_INVALID_ARGUMENT, "edits[%zu].add_sorted is NULL", i);
            for (size_t k = 1; k < e.n_remove; k++)
                AH_REQUIRE(e.remove_sorted[k - 1] < e.remove_sorted[k], AH_ERR_INVALID_ARGUMENT,
                           "edits[%zu].remove_sorted is not strictly ascending at position %zu (%u after %u)", i, k, e.remove_sorted[k],
                           e.remove_sorted[k - 1]);
            for (size_t k = 1; k < e.n_add; k++)
                AH_REQUIRE(e.add_sorted[k - 1] < e.add_sorted[k], AH_ERR_INVALID_ARGUMENT,
                           "edits[%zu].add_sorted is not strictly ascending at position %zu (%u after %u)", i, k, e.add_sorted[k],
                           e.add_sorted[k - 1]);
            n_edit_ids += (uint64_t)e.n_remove + e.n_add;
        }
    for (size_t i = 0; i < n; i++) AH_REQUIRE(filters[i], AH_ERR_INVALID_ARGUMENT, "filters[%zu] is NULL", i);
    ah_index *ix = filters[0]->ix;
    for (size_t i = 1; i < n; i++)
        AH_REQUIRE(filters[i]->ix == ix, AH_ERR_INVALID_ARGUMENT, "filters[%zu] belongs to another index than filters[0]", i);
    AH_TRY(filter_index_live(ix));
    for (size_t i = 0; i < n; i++)
        AH_REQUIRE(filters[i]->suspended, AH_ERR_INVALID_ARGUMENT, "filters[%zu] is not suspended (ah_filter_suspend)", i);
    {
        std::vector<std::pair<const ah_filter *, size_t>> seen(n);
        for (size_t i = 0; i < n; i++) seen[i] = {filters[i], i};
        std::sort(seen.begin(), seen.end());
        for (size_t i = 1; i < n; i++)
            AH_REQUIRE(seen[i].first != seen[i - 1].first, AH_ERR_INVALID_ARGUMENT, "filters[%zu] names the same filter as filters[%zu]",
                       seen[i].second, seen[i - 1].second);
    }
    FilterCall call(ix);
    const FilterBlock &fb = call.fb;
    ah_dataset *ds = call.ds;
    const uint32_t n_nodes = ix->n_nodes;
    const GroupPlan gp(fb);
    const size_t group = gp.group, mixed_bytes = gp.mixed_bytes, n_groups = gp.groups_of(n);
    // the call's one upload: [counters][slots][the edit ids, list after list]
    const size_t counters_bytes = (FC_TOTALS + FC_PER_FILTER * n) * 8, slots_bytes = n * sizeof(CallFilter);
    std::vector<unsigned long long> h((FC_TOTALS + FC_PER_FILTER * n));
    std::vector<uint8_t> up(slots_bytes + (size_t)n_edit_ids * 4);
    AH_TRY(call.begin(n, false));  // (the handles stay the caller's)
    std::vector<DevMem> &blocks = call.blocks;
    DevMem work, mixed;
    if (group > 1 && n_nodes) AH_HIP(dev_malloc(&mixed.p, mixed_bytes));
    AH_HIP(dev_malloc(&work.p, counters_bytes + up.size()));
    unsigned long long *d_counters = work.as<unsigned long long>();
    const CallFilter *d_slots = reinterpret_cast<const CallFilter *>(work.as<uint8_t>() + counters_bytes);
    const uint32_t *d_edit_ids = reinterpret_cast<const uint32_t *>(work.as<uint8_t>() + counters_bytes + slots_bytes);
    {
        CallFilter *slots = reinterpret_cast<CallFilter *>(up.data());
        uint32_t *ids = reinterpret_cast<uint32_t *>(up.data() + slots_bytes);
        uint64_t at = 0;
        for (size_t i = 0; i < n; i++) {
            const ah_filter_edit e = edits ? edits[i] : ah_filter_edit{nullptr, 0, nullptr, 0};
            slots[i] = CallFilter{filters[i]->d_bits, filters[i]->len_bits, blocks[i].as<uint32_t>(), at, e.n_remove, at + e.n_remove, e.n_add};
            if (e.n_remove) memcpy(ids + at, e.remove_sorted, e.n_remove * 4);
            if (e.n_add) memcpy(ids + at + e.n_remove, e.add_sorted, e.n_add * 4);
            at += (uint64_t)e.n_remove + e.n_add;
        }
    }
    AH_TRY(call.stream());
    hipStream_t s = call.s;
    AH_HIP(hipMemsetAsync(d_counters, 0, counters_bytes, s));
    AH_HIP(hipMemcpyAsync(work.as<uint8_t>() + counters_bytes, up.data(), up.size(), hipMemcpyHostToDevice, s));
    const bool count_rows = !ds->identity_ids && ds->n;  // identity ids: every set bit is a row
    size_t max_remove = 0, max_add = 0;
    if (edits)
        for (size_t i = 0; i < n; i++) {
            max_remove = std::max(max_remove, edits[i].n_remove);
            max_add = std::max(max_add, edits[i].n_add);
        }
    // blockIdx.y names the filter: at most 65 535 of them a launch, every launch on its own part of the slots and counters
    for (size_t y0 = 0; y0 < n; y0 += 65535) {
        const uint32_t ny = (uint32_t)std::min<size_t>(n - y0, 65535);
        unsigned long long *per_filter = d_counters + FC_PER_FILTER * y0;  // (k_filter_popcount adds FC_TOTALS itself)
        hipLaunchKernelGGL(k_filter_recut, dim3(grid_of(fb.bytes / 4, 1024, 512), ny), dim3(256), 0, s, d_slots + y0, fb.len_bits,
                           (uint64_t)fb.words, (uint64_t)(fb.bytes / 4));
        if (max_remove)
            hipLaunchKernelGGL(k_filter_edit<false>, dim3(grid_of(max_remove, 256, 256), ny), dim3(256), 0, s, d_slots + y0, d_edit_ids,
                               fb.len_bits, d_counters);
        if (max_add)
            hipLaunchKernelGGL(k_filter_edit<true>, dim3(grid_of(max_add, 256, 256), ny), dim3(256), 0, s, d_slots + y0, d_edit_ids, fb.len_bits,
                               d_counters);
        if (fb.words)
            hipLaunchKernelGGL(k_filter_popcount, dim3(grid_of(fb.words / 4, 256, 256), ny), dim3(256), 0, s, d_slots + y0, (uint64_t)fb.words,
                               per_filter);
        if (count_rows)
            hipLaunchKernelGGL(k_filter_stored_rows, dim3(grid_of(ds->n, 256, 256), ny), dim3(256), 0, s, d_slots + y0, (const uint32_t *)nullptr,
                               ds->view().ids, (uint64_t)ds->n, per_filter + FC_TOTALS + FC_STORED, (uint32_t)FC_PER_FILTER);
    }
    launch_leaf_kept_groups(ix, fb, gp, blocks, mixed, d_counters, s);
    AH_TRY(call.finish(h.data(), d_counters, h.size()));
    // the hand-over: nothing below can fail
    NoFailScope no_fail;
    for (size_t i = 0; i < n; i++) {
        ah_filter *f = filters[i];
        (void)dev_free(f->d_bits);  // (the old block; no kernel reads it any more)
        f->len_bits = fb.len_bits;
        f->listed = h[FC_TOTALS + FC_PER_FILTER * i + FC_LISTED];
        f->stored = count_rows ? h[FC_TOTALS + FC_PER_FILTER * i + FC_STORED] : f->listed;
        f->d_bits = blocks[i].as<uint32_t>();
        f->d_leaf_kept = f->d_bits + fb.words;
        f->device_bytes = dev_block_bytes(blocks[i].p);
        f->suspended = false;
        blocks[i].p = nullptr;
    }
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->filters_suspended -= std::min<uint64_t>(ix->filters_suspended, n);
        ix->fstats.filters_alive += n;
        ix->fstats.leaf_kept_passes += n_nodes ? n_groups : 0;
    }
    if (out_stats)
        *out_stats = ah_filter_resume_stats{n, n_groups, (uint64_t)fb.words * n, h[FC_REMOVED], h[FC_ADDED], h[FC_LEAVES], h[FC_IDS_WALKED]};
    return AH_OK;
    AH_GUARDED_END
}

// ---- filters from serialized RoaringBitmaps (include/arroy_hip.h) ---------------------------------------------------------

// The headers of every blob are judged on the host (roaring_parse.h) before the index is looked at.  Then everything is obtained
// — the n handles and blocks, the call's one device buffer [counters][error word][slots][items][payloads], the interleave
// buffer, the pinned staging — and queued on the calling thread's leased context: a memset per block, ONE upload, k_roaring_expand
// over the travelling containers of the whole call, `stored` on sparse ids, the grouped per-node counts.  One synchronisation;
// the filters join their index after it, where nothing can fail any more.
static int filter_create_roaring(ah_index *ix, const uint8_t *const *blobs, const size_t *lens, size_t n, ah_filter **out,
                                 ah_filter_roaring_stats *out_stats) {
    if (out_stats) *out_stats = ah_filter_roaring_stats{};
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    for (size_t i = 0; i < n; i++) out[i] = nullptr;
    if (n == 0) return AH_OK;
    AH_REQUIRE(blobs && lens, AH_ERR_INVALID_ARGUMENT, "%s is NULL", blobs ? "lens" : "blobs");
    AH_REQUIRE(n < (1u << 24), AH_ERR_INVALID_ARGUMENT, "too many blobs (%zu)", n);
    for (size_t i = 0; i < n; i++) AH_REQUIRE(blobs[i], AH_ERR_INVALID_ARGUMENT, "blobs[%zu] is NULL", i);
    std::vector<std::vector<roaring::Container>> parsed(n);
    std::vector<uint64_t> listed(n);
    for (size_t i = 0; i < n; i++) {
        char why[200];
        AH_REQUIRE(roaring::parse(blobs[i], lens[i], parsed[i], &listed[i], why, sizeof why), AH_ERR_INVALID_ARGUMENT, "blobs[%zu]: %s", i, why);
    }
    AH_TRY(filter_index_live(ix));
    FilterCall call(ix);
    const FilterBlock &fb = call.fb;
    ah_dataset *ds = call.ds;
    const GroupPlan gp(fb);
    const size_t n_groups = gp.groups_of(n);
    // what travels: the containers whose span begins below len_bits, each at a 16-byte boundary of the staging and in whole
    // 16-byte units
    ah_filter_roaring_stats st{};
    st.filters = n, st.groups = n_groups;
    std::vector<RoaringItem> items;
    uint64_t staging_bytes = 0;
    for (size_t i = 0; i < n; i++)
        for (size_t c = 0; c < parsed[i].size(); c++) {
            const roaring::Container &k = parsed[i][c];
            if (fb.len_bits == 0 || k.key > ((fb.len_bits - 1) >> 16)) {
                st.skipped_containers++;
                continue;
            }
            (k.kind == roaring::KIND_ARRAY ? st.array_containers : k.kind == roaring::KIND_BITMAP ? st.bitmap_containers : st.run_containers)++;
            st.bytes_uploaded += k.bytes;
            items.push_back(RoaringItem{(uint32_t)i, (uint32_t)c, k.key, k.kind, k.cardinality, k.n_runs, staging_bytes});
            staging_bytes += (k.bytes + 15) & ~(uint64_t)15;
        }
    AH_REQUIRE(items.size() < 0x7FFFFFFFull, AH_ERR_INVALID_ARGUMENT, "too many containers (%zu)", items.size());
    // the call's one device buffer: [counters][error word (8)][slots][items][payloads], every part a multiple of 16 bytes
    const size_t err_word = (FC_TOTALS + FC_PER_FILTER * n + 1) & ~(size_t)1, counters_bytes = (err_word + 2) * 8;
    const size_t slots_bytes = (n * sizeof(CallFilter) + 15) & ~(size_t)15, items_bytes = items.size() * sizeof(RoaringItem);
    const size_t up_bytes = slots_bytes + items_bytes + (size_t)staging_bytes;
    std::vector<unsigned long long> h(err_word + 2);
    AH_TRY(call.begin(n));
    std::vector<DevMem> &blocks = call.blocks;
    DevMem work, mixed;
    if (gp.group > 1 && n > 1 && ix->n_nodes) AH_HIP(dev_malloc(&mixed.p, gp.mixed_bytes));  // (one filter: a pass on its own bitmap)
    AH_HIP(dev_malloc(&work.p, counters_bytes + up_bytes));
    AH_TRY(call.stream());
    Context *ctx = call.lease->c;
    AH_TRY(ctx->ensure_pinned(up_bytes));
    hipStream_t s = call.s;
    unsigned long long *d_counters = work.as<unsigned long long>();
    uint8_t *d_up = work.as<uint8_t>() + counters_bytes;
    const CallFilter *d_slots = reinterpret_cast<const CallFilter *>(d_up);
    const RoaringItem *d_items = reinterpret_cast<const RoaringItem *>(d_up + slots_bytes);
    const uint8_t *d_staging = d_up + slots_bytes + items_bytes;
    {
        uint8_t *pin = reinterpret_cast<uint8_t *>(ctx->h_pinned);
        CallFilter *slots = reinterpret_cast<CallFilter *>(pin);
        for (size_t i = 0; i < n; i++) slots[i] = CallFilter{nullptr, 0, blocks[i].as<uint32_t>(), 0, 0, 0, 0};
        if (!items.empty()) memcpy(pin + slots_bytes, items.data(), items_bytes);
        uint8_t *staging = pin + slots_bytes + items_bytes;
        for (const RoaringItem &it : items) {
            const roaring::Container &k = parsed[it.filter][it.container];
            memcpy(staging + it.payload, blobs[it.filter] + k.offset, (size_t)k.bytes);
            const size_t pad = (size_t)(((k.bytes + 15) & ~(uint64_t)15) - k.bytes);
            if (pad) memset(staging + it.payload + k.bytes, 0, pad);
        }
    }
    AH_HIP(hipMemsetAsync(d_counters, 0, err_word * 8, s));
    AH_HIP(hipMemsetAsync(d_counters + err_word, 0xFF, 16, s));  // (the error word: "nothing found")
    for (size_t i = 0; i < n; i++) AH_HIP(hipMemsetAsync(blocks[i].p, 0, fb.bytes, s));
    AH_HIP(hipMemcpyAsync(d_up, ctx->h_pinned, up_bytes, hipMemcpyHostToDevice, s));
    if (!items.empty())
        hipLaunchKernelGGL(k_roaring_expand, dim3((uint32_t)items.size()), dim3(256), 0, s, d_items, d_staging, d_slots, fb.len_bits, d_counters,
                           d_counters + err_word);
    const bool count_rows = !ds->identity_ids && ds->n;  // identity ids: every bit below len_bits = n is a row
    if (count_rows)
        for (size_t y0 = 0; y0 < n; y0 += 65535)  // (blockIdx.y names the filter)
            hipLaunchKernelGGL(k_filter_stored_rows, dim3(grid_of(ds->n, 256, 256), (uint32_t)std::min<size_t>(n - y0, 65535)), dim3(256), 0, s,
                               d_slots + y0, (const uint32_t *)nullptr, ds->view().ids, (uint64_t)ds->n,
                               d_counters + FC_TOTALS + FC_PER_FILTER * y0 + FC_STORED, (uint32_t)FC_PER_FILTER);
    launch_leaf_kept_groups(ix, fb, gp, blocks, mixed, d_counters, s);
    AH_TRY(call.finish(h.data(), d_counters, h.size()));
    if (h[err_word] != ~0ull) {
        static const char *const kWhy[] = {"", "the array does not ascend strictly", "the bitmap's popcount is not the cardinality",
                                           "the runs overlap or are out of order", "a run reaches past 65535",
                                           "the runs' total length is not the cardinality"};
        const unsigned reason = (unsigned)(h[err_word] & 0xFF);
        AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "blobs[%llu]: container %llu: %s", h[err_word] >> 24, (h[err_word] >> 8) & 0xFFFF,
                   reason < sizeof kWhy / sizeof kWhy[0] ? kWhy[reason] : "malformed");
    }
    // the hand-over: nothing below can fail
    NoFailScope no_fail;
    for (size_t i = 0; i < n; i++) {
        const uint64_t inside = h[FC_TOTALS + FC_PER_FILTER * i + FC_LISTED];
        call.adopt(i, listed[i], count_rows ? h[FC_TOTALS + FC_PER_FILTER * i + FC_STORED] : inside, i == 0 ? n_groups : 0, &out[i]);
    }
    st.leaves = h[FC_LEAVES], st.ids_walked = h[FC_IDS_WALKED];
    if (out_stats) *out_stats = st;
    return AH_OK;
}

int ah_filter_create_roaring_batch(ah_index *ix, const uint8_t *const *blobs, const size_t *lens, size_t n, ah_filter **out,
                                   ah_filter_roaring_stats *out_stats) {
    AH_GUARDED("ah_filter_create_roaring_batch")
    return filter_create_roaring(ix, blobs, lens, n, out, out_stats);
    AH_GUARDED_END
}

// The batch of one.
int ah_filter_create_roaring(ah_index *ix, const uint8_t *bytes, size_t len, ah_filter **out) {
    AH_GUARDED("ah_filter_create_roaring")
    return filter_create_roaring(ix, &bytes, &len, 1, out, nullptr);
    AH_GUARDED_END
}

int ah_index_filter_stats(ah_index *ix, ah_filter_stats *out, int reset) {
    AH_GUARDED("ah_index_filter_stats")
    AH_REQUIRE(ix && out, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    *out = ix->fstats;
    if (reset) {
        const uint64_t alive = ix->fstats.filters_alive;
        ix->fstats = ah_filter_stats{};
        ix->fstats.filters_alive = alive;
    }
    return AH_OK;
    AH_GUARDED_END
}

// kept_total(f) (include/arroy_hip.h): made on first request, cached until the filter is suspended.
int ah_filter_kept_total(ah_filter *f, uint64_t *out) {
    AH_GUARDED("ah_filter_kept_total")
    AH_REQUIRE(f && f->ix && f->ix->ds, AH_ERR_INVALID_ARGUMENT, "filter is NULL");
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    AH_REQUIRE(!f->suspended, AH_ERR_INVALID_ARGUMENT, "the filter is suspended (ah_filter_suspend): ah_filter_resume_batch it first");
    AH_INDEX_LIVE(f->ix);
    ah_dataset *ds = f->ix->ds;
    AH_HIP(hipSetDevice(ds->device));
    ContextLease lease(ds);
    AH_REQUIRE(lease.c, AH_ERR_DEVICE, "cannot create a HIP stream");
    return filter_kept_total(f, lease.c, *out);
    AH_GUARDED_END
}

// Test aid: K(f) as the exhausted queries of the filter read it.
int ah_filter_kept_ids(ah_filter *f, uint32_t *out_ids, uint64_t cap, uint64_t *out_n) {
    AH_GUARDED("ah_filter_kept_ids")
    AH_REQUIRE(f && f->ix && f->ix->ds, AH_ERR_INVALID_ARGUMENT, "filter is NULL");
    AH_REQUIRE(out_n, AH_ERR_INVALID_ARGUMENT, "out_n is NULL");
    AH_REQUIRE(!f->suspended, AH_ERR_INVALID_ARGUMENT, "the filter is suspended (ah_filter_suspend): ah_filter_resume_batch it first");
    AH_INDEX_LIVE(f->ix);
    ah_dataset *ds = f->ix->ds;
    AH_HIP(hipSetDevice(ds->device));
    ContextLease lease(ds);
    AH_REQUIRE(lease.c, AH_ERR_DEVICE, "cannot create a HIP stream");
    AH_TRY(filter_kept_list(f, lease.c));
    *out_n = f->n_list;
    if (out_ids && f->n_list) {
        AH_REQUIRE(cap >= f->n_list, AH_ERR_INVALID_ARGUMENT, "cap = %llu is below the list's %llu ids", (unsigned long long)cap,
                   (unsigned long long)f->n_list);
        AH_HIP(hipMemcpyAsync(out_ids, f->d_list, (size_t)f->n_list * 4, hipMemcpyDeviceToHost, lease.c->stream));
        AH_HIP(hipStreamSynchronize(lease.c->stream));
    }
    return AH_OK;
    AH_GUARDED_END
}

}  // extern "C"
