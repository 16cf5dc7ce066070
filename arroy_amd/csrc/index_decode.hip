// index_decode.hip — ah_index_create_from_encoded (include/arroy_hip.h): a resident index from the bytes LMDB stores for the
// tree nodes (node_decode.h), the inverse of encode.hip.  The host copies every value into the call's pinned buffer and reads
// none of its bytes; the device measures, links, unpacks and expands them ("Opening a resident index from encoded
// nodes").
//
//   measure   one wavefront per value: tag, length, children (big-endian), and for a Descendants value the Roaring headers —
//             the containers dealt over the lanes, their sizes prefix-summed against the offset header; a value the lanes
//             find at fault is judged again by the serial measure_value of node_decode.h, whose reason is the one reported
//   scan      the id counts and the has_normal flags of a chunk become first ids and normal rows (scan_device.h)
//   links     one thread per value: children -> ranks among node_ids (binary search), first id, normal row
//   normals   one wavefront per split value with a plane: header and vector lie at byte 9 of a 16-byte aligned value, so
//             every word is funnelled out of two aligned loads
//   expand    Descendants: one wavefront per value whose containers are all arrays (ids dealt flat over the lanes, the
//             container of an output position found in the prefix of the cardinalities in LDS); one block per value with a
//             bitmap or run container, container after container
//
// Nothing indexes memory by an unchecked value: the expansion runs only on chunks whose headers the measure pass accepted,
// and every write lands inside [DNode.a, DNode.a + DNode.b) of its node.
//
// ah_index_create_from_legacy is the same call behind a layout (node_legacy.h: the split values of arroy v0.4 - v0.6, with
// NodeId children that may be items, a normal that is never absent and no header).  The passes differ as follows:
//   measure   a split value's head by measure_split_head, its vector by a wave-wide is_zero (f32: the sign bit masked)
//   scan      a third scan, of the Item children: it carries on across chunks and gives every new one-id Descendants node its
//             slot behind the nodes of the values
//   links     an Item child becomes that slot; its id is kept for the end of the call
//   normals   the rows are funnelled from byte 11; the headers are made of the rows by launch_headers_from_vectors, the
//             `D::new_header` code of ah_dataset_upload_vectors
//   the end   k_dec_new_nodes writes the new nodes and appends their ids to the descendants
#include <memory>

#include "index_device.h"
#include "node_decode.h"
#include "node_legacy.h"
#include "scan_device.h"

namespace ah {
namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kDecBlock = 256;
constexpr uint32_t kWaveMaxContainers = 1024;  // containers whose cardinality prefix a wave of the expansion keeps in LDS
constexpr uint32_t kNone = 0xFFFFFFFFu;

// One staged value: which node it is, and where its bytes lie in the chunk's staging buffer.  The host puts every value at
// a 16-byte boundary and allots it whole 16-byte units (zeroed behind the value), so an aligned 4-byte load that begins
// inside a value ends inside its allotment.
struct DecValue {
    uint32_t node;    // position among node_ids = index of the node
    uint32_t len;
    uint64_t offset;  // from the start of the staging buffer, a multiple of 16
};
static_assert(sizeof(DecValue) == 16, "laid out by hand in the chunk's one upload");

// the chunk's control block: 64-bit words, then the totals of the scans
enum DecWord : uint32_t {
    DW_ERR,  // the smallest (node position << 8) | reason; ~0: nothing found
    DW_IDS,
    DW_ARRAYS,
    DW_BITMAPS,
    DW_RUNS,
    DW_SPLITS,
    DW_NORMALS,
    DW_LEAVES,
    DW_WAVE_VALUES,
    DW_BLOCK_VALUES,
    DW_BLOCK_CONTAINERS,
    DW_ITEMS,  // legacy layouts: Item children = new one-id Descendants nodes
    DW_ZEROS,  // legacy layouts: split values whose vector is_zero accepts
    DW_WORDS
};
struct DecCtl {
    unsigned long long w[DW_WORDS];
    uint32_t ids_total, normals_total;  // of the chunk, from the scans (32 bits: the host trusts w[DW_IDS])
    uint32_t items_total, reserved;
};
constexpr uint32_t kLeftItem = 0x200u, kRightItem = 0x400u;  // DNode.kind between measure and links: that child is an Item id
constexpr uint32_t kInfoBlock = 0x80000000u;  // info[i]: this Descendants value takes the block path of the expansion

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ void refuse(DecCtl *ctl, uint32_t node, uint32_t reason) {
    atomicMin(&ctl->w[DW_ERR], ((unsigned long long)node << 8) | reason);
}
// the position of `id` in ids[0, n) (ascending), or kNone
__device__ __forceinline__ uint32_t rank_of(const uint32_t *__restrict__ ids, uint32_t n, uint32_t id) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && ids[lo] == id ? lo : kNone;
}
// the 32-bit word at byte `at` of a 16-byte aligned value, out of the aligned words around it
__device__ __forceinline__ uint32_t word_at(const uint8_t *v, uint64_t at) {
    const uint32_t *a = reinterpret_cast<const uint32_t *>(v) + (at >> 2);
    const uint32_t sh = 8u * (uint32_t)(at & 3);
    return sh ? __builtin_amdgcn_alignbit(a[1], a[0], sh) : a[0];
}

// ---- measure -------------------------------------------------------------------------------------------------------------------
// Values [first, first + n) of the chunk.  nodes[value.node] gets {kind | has_normal << 8, raw left, raw right, 0} or
// {Descendants, 0, count, 0}, a refused value {0, 0, 0, 0}; cnt / nrm / info are indexed by the value's place in the chunk.
// A legacy layout (node_legacy.h): a split value is [2][NodeId][NodeId][vector]; its head is judged by measure_split_head, its
// vector by the wave (has_normal = some word is not zero), kLeftItem / kRightItem mark the Item children for the links pass
// and itm gets their number.
__global__ __launch_bounds__(kDecBlock) void k_dec_measure(const uint8_t *__restrict__ staging, const DecValue *__restrict__ vals, uint32_t first,
                                                          uint32_t n, int layout, uint32_t f32, uint32_t header_size, uint32_t vector_size,
                                                          DNode *__restrict__ nodes, uint32_t *__restrict__ cnt, uint32_t *__restrict__ nrm,
                                                          uint32_t *__restrict__ info, uint32_t *__restrict__ itm, DecCtl *__restrict__ ctl) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t n_waves = gridDim.x * (kDecBlock / kWave);
    unsigned long long t_ids = 0;
    uint32_t t_arrays = 0, t_bitmaps = 0, t_runs = 0, t_splits = 0, t_normals = 0, t_leaves = 0, t_wave = 0, t_block = 0, t_block_c = 0, t_items = 0, t_zeros = 0;
    for (uint32_t i = first + (blockIdx.x * kDecBlock + threadIdx.x) / kWave; i < first + n; i += n_waves) {
        const DecValue dv = vals[i];
        const uint8_t *v = staging + dv.offset;
        const uint64_t len = dv.len;
        decode::Measured m{};
        bool serial = true;  // the serial reference judges the value: every split value, every value the lanes find at fault
        if (len >= 1 && v[0] == codec::kTagDescendants) {
            const uint8_t *ser = v + 1;
            const uint64_t slen = len - 1;
            decode::Header h;
            if (decode::read_header(ser, slen, &h) == decode::R_OK && h.offsets_at) {
                // container c's place is what its offset entry states; the sizes read there, prefix-summed, must give the same
                // place — for the first container that is `headers`, and by induction every entry is then the true one
                bool bad = false;
                uint64_t carry = h.headers, ids = 0;
                uint32_t arrays = 0, bitmaps = 0, runs = 0;
                for (uint64_t base = 0; base < h.nc; base += kWave) {
                    const uint64_t c = base + lane;
                    uint32_t size = 0;
                    uint64_t stated = 0;
                    if (c < h.nc) {
                        const uint32_t key = decode::get_le16(ser + h.pairs_at + 4 * c), card = decode::get_le16(ser + h.pairs_at + 4 * c + 2) + 1;
                        if (c && key <= decode::get_le16(ser + h.pairs_at + 4 * (c - 1))) bad = true;
                        stated = decode::get_le32(ser + h.offsets_at + 4 * c);
                        if (decode::is_run(ser, h, c)) {
                            runs++;
                            if (stated + 2 > slen) bad = true;
                            else size = 2 + 4 * decode::get_le16(ser + stated);
                        } else if (card <= roaring::kArrayMax) {
                            arrays++;
                            size = 2 * card;
                        } else {
                            bitmaps++;
                            size = roaring::kBitmapBytes;
                        }
                        ids += card;
                    }
                    const uint32_t incl = wave_inclusive_sum(size);  // (64 x at most 262 142 bytes)
                    const uint64_t pos = carry + incl - size;
                    if (c < h.nc && (stated != pos || pos + size > slen)) bad = true;
                    carry += __shfl(incl, kWave - 1, kWave);
                }
                if (!__any(bad) && carry == slen) {
                    serial = false;
                    m.kind = codec::kTagDescendants;
                    m.ids = wave_sum_u64(ids);
                    m.arrays = (uint32_t)wave_sum_u64(arrays);
                    m.bitmaps = (uint32_t)wave_sum_u64(bitmaps);
                    m.runs = (uint32_t)wave_sum_u64(runs);
                    m.containers = (uint32_t)h.nc;
                    m.reason = m.ids > 0xFFFFFFFFull ? decode::R_TOO_MANY_IDS : decode::R_OK;
                }
            }
        }
        uint32_t item_bits = 0;
        if (serial && layout != legacy::L_V0_7 && len >= 1 && v[0] == codec::kTagSplit) {
            const legacy::Measured lm = legacy::measure_split_head(v, len, layout, vector_size);  // (every lane the same)
            m = lm.m;
            if (m.reason == decode::R_OK) {
                bool some = false;  // the wave-wide is_zero: len is 11 + vector_size, so every word lies inside the value
                for (uint32_t w = lane; w < vector_size / 4; w += kWave)
                    some |= !legacy::word_is_zero(word_at(v, legacy::kSplitHead + 4ull * w), f32 != 0);
                m.has_normal = __any(some) ? 1u : 0u;
                item_bits = (lm.left_is_item ? kLeftItem : 0u) | (lm.right_is_item ? kRightItem : 0u);
            }
        } else if (serial) {
            m = decode::measure_value(v, len, header_size, vector_size);  // (every lane the same)
        }
        if (lane != 0) continue;
        DNode d{0, 0, 0, 0};
        uint32_t count = 0, normal = 0, inf = 0, items = 0;
        if (m.reason != decode::R_OK) {
            refuse(ctl, dv.node, m.reason);
        } else if (m.kind == codec::kTagSplit) {
            d = DNode{AH_NODE_SPLIT | (m.has_normal ? 0x100u : 0u) | item_bits, m.left, m.right, 0};
            normal = m.has_normal;
            items = (uint32_t)__popc(item_bits);
            t_splits++;
            t_normals += normal;
            t_items += items;
            if (layout != legacy::L_V0_7) t_zeros += 1u - normal;
        } else {
            count = (uint32_t)m.ids;
            d = DNode{AH_NODE_DESCENDANTS, 0, count, 0};
            inf = m.containers;
            t_leaves++;
            t_ids += m.ids;
            t_arrays += m.arrays, t_bitmaps += m.bitmaps, t_runs += m.runs;
            if (m.bitmaps || m.runs || m.containers > kWaveMaxContainers) {
                inf |= kInfoBlock;
                t_block++;
                t_block_c += m.containers;
            } else {
                t_wave++;
            }
        }
        nodes[dv.node] = d;
        cnt[i] = count;
        nrm[i] = normal;
        info[i] = inf;
        if (itm) itm[i] = items;
    }
    if (lane == 0) {
        if (t_ids) atomicAdd(&ctl->w[DW_IDS], t_ids);
        if (t_arrays) atomicAdd(&ctl->w[DW_ARRAYS], (unsigned long long)t_arrays);
        if (t_bitmaps) atomicAdd(&ctl->w[DW_BITMAPS], (unsigned long long)t_bitmaps);
        if (t_runs) atomicAdd(&ctl->w[DW_RUNS], (unsigned long long)t_runs);
        if (t_splits) atomicAdd(&ctl->w[DW_SPLITS], (unsigned long long)t_splits);
        if (t_normals) atomicAdd(&ctl->w[DW_NORMALS], (unsigned long long)t_normals);
        if (t_leaves) atomicAdd(&ctl->w[DW_LEAVES], (unsigned long long)t_leaves);
        if (t_wave) atomicAdd(&ctl->w[DW_WAVE_VALUES], (unsigned long long)t_wave);
        if (t_block) atomicAdd(&ctl->w[DW_BLOCK_VALUES], (unsigned long long)t_block);
        if (t_block_c) atomicAdd(&ctl->w[DW_BLOCK_CONTAINERS], (unsigned long long)t_block_c);
        if (t_items) atomicAdd(&ctl->w[DW_ITEMS], (unsigned long long)t_items);
        if (t_zeros) atomicAdd(&ctl->w[DW_ZEROS], (unsigned long long)t_zeros);
    }
}

// ---- links: children -> ranks, first ids, normal rows (cnt / nrm / itm hold the exclusive prefixes of the chunk by now) ---------
// An Item child becomes new node item_base + its place among the Item children of the chunk, slot n_nodes + that, left before
// right; its id goes to new_items at its place in the chunk (room for two per value).
__global__ __launch_bounds__(kDecBlock) void k_dec_links(const DecValue *__restrict__ vals, uint32_t n, const uint32_t *__restrict__ node_ids,
                                                        uint32_t n_nodes, DNode *__restrict__ nodes, const uint32_t *__restrict__ cnt,
                                                        const uint32_t *__restrict__ nrm, const uint32_t *__restrict__ itm, uint32_t desc_base,
                                                        uint32_t row_base, uint32_t item_base, uint32_t *__restrict__ new_items,
                                                        DecCtl *__restrict__ ctl) {
    const uint32_t stride = gridDim.x * kDecBlock;
    for (uint32_t i = blockIdx.x * kDecBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t node = vals[i].node;
        DNode d = nodes[node];
        if ((d.kind & 0xFFu) == AH_NODE_SPLIT) {
            uint32_t place = itm ? itm[i] : 0u, left, right;
            if (d.kind & kLeftItem) {
                new_items[place] = d.a;
                left = n_nodes + item_base + place++;
            } else {
                left = rank_of(node_ids, n_nodes, d.a);
            }
            if (d.kind & kRightItem) {
                new_items[place] = d.b;
                right = n_nodes + item_base + place;
            } else {
                right = rank_of(node_ids, n_nodes, d.b);
            }
            if (left == kNone || right == kNone) refuse(ctl, node, decode::R_CHILD_ABSENT);
            d.kind &= ~(kLeftItem | kRightItem);
            d.a = left, d.b = right;
            d.c = (d.kind & 0x100u) ? row_base + nrm[i] : 0u;
        } else if (d.kind == AH_NODE_DESCENDANTS) {
            d.a = desc_base + cnt[i];
        }
        nodes[node] = d;
    }
}
// the root ids, in place; w[DW_ERR] of `ctl` names the tree position
__global__ __launch_bounds__(kDecBlock) void k_dec_roots(uint32_t *__restrict__ roots, uint32_t n_trees, const uint32_t *__restrict__ node_ids,
                                                        uint32_t n_nodes, DecCtl *__restrict__ ctl) {
    const uint32_t stride = gridDim.x * kDecBlock;
    for (uint32_t t = blockIdx.x * kDecBlock + threadIdx.x; t < n_trees; t += stride) {
        const uint32_t r = rank_of(node_ids, n_nodes, roots[t]);
        if (r == kNone) refuse(ctl, t, decode::R_ROOT_ABSENT);
        else roots[t] = r;
    }
}

// the one-id Descendants nodes of the Item children, behind the nodes and the lists of the values: new node j holds items[j]
__global__ __launch_bounds__(kDecBlock) void k_dec_new_nodes(const uint32_t *__restrict__ items, uint32_t n, uint32_t desc_base,
                                                            DNode *__restrict__ new_nodes, uint32_t *__restrict__ new_desc) {
    const uint32_t stride = gridDim.x * kDecBlock;
    for (uint32_t j = blockIdx.x * kDecBlock + threadIdx.x; j < n; j += stride) {
        new_nodes[j] = DNode{AH_NODE_DESCENDANTS, desc_base + j, 1, 0};
        new_desc[j] = items[j];
    }
}

// ---- normals: what k_unpack_normals writes, out of [2][left][right][header][vector] (head = 9, hf header words copied) or out
// of the legacy [2][NodeId][NodeId][vector] (head = 11, hf = 0: the headers are made of the rows afterwards) ---------------------
__global__ __launch_bounds__(kDecBlock) void k_dec_normals(const uint8_t *__restrict__ staging, const DecValue *__restrict__ vals, uint32_t first,
                                                          uint32_t n, const DNode *__restrict__ nodes, uint32_t head, uint32_t header_size,
                                                          uint32_t hf, uint32_t valid_words32, uint32_t row_words32, uint32_t rows_cap,
                                                          uint32_t *__restrict__ rows, float *__restrict__ headers) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t n_waves = gridDim.x * (kDecBlock / kWave);
    for (uint32_t i = first + (blockIdx.x * kDecBlock + threadIdx.x) / kWave; i < first + n; i += n_waves) {
        const DecValue dv = vals[i];
        const DNode d = nodes[dv.node];
        if (d.kind != (AH_NODE_SPLIT | 0x100u) || d.c >= rows_cap) continue;
        const uint8_t *v = staging + dv.offset;
        const uint64_t vec = head + header_size;
        for (uint32_t w = lane; w < row_words32; w += kWave)
            rows[(uint64_t)d.c * row_words32 + w] = w < valid_words32 ? word_at(v, vec + 4ull * w) : 0u;
        if (lane < hf) headers[(uint64_t)d.c * hf + lane] = __uint_as_float(word_at(v, head + 4ull * lane));
    }
}

// ---- Descendants, every container an array: the low 16 bits of id p lie at `headers` + 2 p -----------------------------------
__global__ __launch_bounds__(kDecBlock) void k_dec_desc_wave(const uint8_t *__restrict__ staging, const DecValue *__restrict__ vals, uint32_t first,
                                                            uint32_t n, const DNode *__restrict__ nodes, const uint32_t *__restrict__ info,
                                                            uint32_t *__restrict__ desc, uint64_t desc_cap, DecCtl *__restrict__ ctl) {
    __shared__ uint32_t s_prefix[kDecBlock / kWave][kWaveMaxContainers + 1];
    const uint32_t lane = threadIdx.x & (kWave - 1);
    uint32_t *prefix = s_prefix[threadIdx.x / kWave];
    const uint32_t n_waves = gridDim.x * (kDecBlock / kWave);
    for (uint32_t i = first + (blockIdx.x * kDecBlock + threadIdx.x) / kWave; i < first + n; i += n_waves) {
        const DecValue dv = vals[i];
        const DNode d = nodes[dv.node];
        if (d.kind != AH_NODE_DESCENDANTS || (info[i] & kInfoBlock) || d.b == 0) continue;
        const uint8_t *ser = staging + dv.offset + 1;
        decode::Header h;
        (void)decode::read_header(ser, dv.len - 1, &h);
        const uint32_t nc = min((uint32_t)h.nc, kWaveMaxContainers);
        uint32_t carry = 0;
        for (uint32_t base = 0; base < nc; base += kWave) {
            const uint32_t c = base + lane;
            const uint32_t card = c < nc ? decode::get_le16(ser + h.pairs_at + 4ull * c + 2) + 1 : 0u;
            const uint32_t incl = wave_inclusive_sum(card);
            if (c < nc) prefix[c] = carry + incl - card;
            carry += __shfl(incl, kWave - 1, kWave);
        }
        if (lane == 0) prefix[nc] = carry;
        wave_sync();
        const uint32_t count = min(carry, d.b);  // (equal: the measure pass summed the same cardinalities)
        const uint8_t *body = ser + h.headers;
        bool bad = false;
        for (uint32_t base = 0; base < count; base += kWave) {
            const uint32_t p = base + lane;
            const bool valid = p < count;
            const uint32_t low = valid ? decode::get_le16(body + 2ull * p) : 0u;
            uint32_t prev = __shfl_up(low, 1, kWave);
            if (lane == 0 && valid && p) prev = decode::get_le16(body + 2ull * (p - 1));  // (the last id of the step before)
            if (!valid) continue;
            uint32_t lo = 0, hi = nc;  // the last container that begins at or before p
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (prefix[mid] <= p) lo = mid;
                else hi = mid;
            }
            if (p > prefix[lo] && low <= prev) bad = true;
            if ((uint64_t)d.a + p < desc_cap) desc[(uint64_t)d.a + p] = decode::get_le16(ser + h.pairs_at + 4ull * lo) << 16 | low;
        }
        if (__any(bad) && lane == 0) refuse(ctl, dv.node, decode::R_ARRAY_ORDER);
        wave_sync();  // (the prefix is the next value's from here)
    }
}

// ---- Descendants with bitmap or run containers (or more containers than a wave's prefix holds): one block per value ----------
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t x, uint32_t *s_wave, uint32_t *total) {
    const uint32_t incl = wave_inclusive_sum(x), wave = threadIdx.x / kWave;
    __syncthreads();  // (s_wave of the scan before)
    if ((threadIdx.x & (kWave - 1)) == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t run = incl - x;
    for (uint32_t w = 0; w < wave; w++) run += s_wave[w];
    *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return run;
}
__global__ __launch_bounds__(kDecBlock) void k_dec_desc_block(const uint8_t *__restrict__ staging, const DecValue *__restrict__ vals, uint32_t first,
                                                             uint32_t n, const DNode *__restrict__ nodes, const uint32_t *__restrict__ info,
                                                             uint32_t *__restrict__ desc, uint64_t desc_cap, DecCtl *__restrict__ ctl) {
    __shared__ uint32_t s_wave[kDecBlock / kWave], s_at[kDecBlock + 1], s_start[kDecBlock], s_bad;
    const uint32_t t = threadIdx.x;
    for (uint32_t i = first + blockIdx.x; i < first + n; i += gridDim.x) {
        const DecValue dv = vals[i];
        const DNode d = nodes[dv.node];
        if (d.kind != AH_NODE_DESCENDANTS || !(info[i] & kInfoBlock)) continue;  // (block-uniform)
        const uint8_t *ser = staging + dv.offset + 1;
        const uint64_t slen = dv.len - 1;
        decode::Header h;
        (void)decode::read_header(ser, slen, &h);
        if (t == 0) s_bad = kNone;
        uint32_t bad = kNone;  // the smallest reason this thread found
        uint64_t pos = h.headers, out_at = d.a;
        const uint64_t out_end = min((uint64_t)d.a + d.b, desc_cap);
        for (uint64_t c = 0; c < h.nc; c++) {
            decode::ContainerAt k;
            (void)decode::container_at(ser, slen, h, c, pos, &k);  // (the measure pass has walked the same containers)
            const uint8_t *p = ser + k.offset;
            const uint32_t high = k.key << 16, card = k.cardinality;
            auto put = [&](uint32_t at, uint32_t low) {  // id `at` of the container
                if (at < card && out_at + at < out_end) desc[out_at + at] = high | low;
            };
            if (k.kind == roaring::KIND_ARRAY) {
                for (uint32_t j = t; j < card; j += kDecBlock) {
                    const uint32_t low = decode::get_le16(p + 2ull * j);
                    if (j && low <= decode::get_le16(p + 2ull * (j - 1))) bad = min(bad, (uint32_t)decode::R_ARRAY_ORDER);
                    put(j, low);
                }
            } else if (k.kind == roaring::KIND_BITMAP) {
                // eight words a thread, funnelled out of nine aligned ones (the payload begins at any address; a ninth word
                // that is read begins inside the payload); ids by popcount rank
                const uintptr_t addr = reinterpret_cast<uintptr_t>(p) + 32u * t;
                const uint32_t *a = reinterpret_cast<const uint32_t *>(addr & ~(uintptr_t)3);
                const uint32_t sh = 8u * (uint32_t)(addr & 3);
                uint32_t w[8], mine = 0, lo = a[0];
#pragma unroll
                for (uint32_t e = 0; e < 8; e++) {
                    const uint32_t hi = (sh || e < 7) ? a[e + 1] : 0u;
                    w[e] = sh ? __builtin_amdgcn_alignbit(hi, lo, sh) : lo;
                    mine += (uint32_t)__popc(w[e]);
                    lo = hi;
                }
                uint32_t total;
                uint32_t at = block_exclusive_sum(mine, s_wave, &total);
                if (total != card) bad = min(bad, (uint32_t)decode::R_BITMAP_CARDINALITY);
#pragma unroll
                for (uint32_t e = 0; e < 8; e++) {
                    uint32_t left = w[e];
                    while (left) {
                        put(at++, (8u * t + e) * 32u + (uint32_t)__ffs((int)left) - 1u);
                        left &= left - 1u;
                    }
                }
            } else {
                // 256 runs a round: their lengths prefix-summed, then the ids of the round dealt flat over the threads
                uint32_t done = 0;
                for (uint32_t r0 = 0; r0 < k.n_runs; r0 += kDecBlock) {
                    const uint32_t r = r0 + t;
                    uint32_t start = 0, length = 0;
                    if (r < k.n_runs) {
                        start = decode::get_le16(p + 2 + 4ull * r);
                        uint32_t end = start + decode::get_le16(p + 4 + 4ull * r);  // inclusive
                        if (end > 0xFFFFu) {
                            bad = min(bad, (uint32_t)decode::R_RUN_PAST_END);
                            end = 0xFFFFu;
                        }
                        if (r && start <= decode::get_le16(p + 2 + 4ull * (r - 1)) + decode::get_le16(p + 4 + 4ull * (r - 1)))
                            bad = min(bad, (uint32_t)decode::R_RUN_ORDER);
                        length = end - start + 1;
                    }
                    uint32_t total;
                    const uint32_t at = block_exclusive_sum(length, s_wave, &total);
                    __syncthreads();  // (s_at / s_start of the round before)
                    s_at[t] = at;
                    s_start[t] = start;
                    if (t == 0) s_at[kDecBlock] = total;
                    __syncthreads();
                    for (uint32_t q = t; q < total; q += kDecBlock) {
                        uint32_t lo = 0, hi = kDecBlock;  // the last run that begins at or before q
                        while (hi - lo > 1) {
                            const uint32_t mid = lo + (hi - lo) / 2;
                            if (s_at[mid] <= q) lo = mid;
                            else hi = mid;
                        }
                        if ((uint64_t)done + q < card) put(done + q, (s_start[lo] + (q - s_at[lo])) & 0xFFFFu);
                    }
                    done = (uint32_t)min((uint64_t)done + total, (uint64_t)kNone);
                }
                if (done != card) bad = min(bad, (uint32_t)decode::R_RUN_CARDINALITY);
            }
            out_at += card;
            pos += k.bytes;
        }
        __syncthreads();  // (s_bad is set)
        if (bad != kNone) atomicMin(&s_bad, bad);
        __syncthreads();
        if (t == 0 && s_bad != kNone) refuse(ctl, dv.node, s_bad);
        __syncthreads();  // (s_bad is the next value's from here)
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int alloc(DevMem *m, size_t bytes) { return ah::alloc(m, bytes, "the index from encoded nodes"); }

// `m` holds at least `need` bytes afterwards (`exact`: just that many, at least one), its first `used` bytes kept
int fit(DevMem *m, uint64_t *cap, uint64_t used, uint64_t need, bool exact, hipStream_t s) {
    need = std::max<uint64_t>(1, need);
    if (m->p && (exact ? *cap == need : *cap >= need)) return AH_OK;
    const uint64_t new_cap = exact ? need : std::max<uint64_t>(need, 2 * *cap);
    DevMem fresh;
    AH_TRY(alloc(&fresh, new_cap));
    if (m->p && used) AH_HIP(hipMemcpyAsync(fresh.p, m->p, std::min(used, new_cap), hipMemcpyDeviceToDevice, s));
    std::swap(m->p, fresh.p);  // (dev_free of the old block waits for the copy)
    *cap = new_cap;
    return AH_OK;
}

struct Chunk {
    size_t lo, hi;   // node positions
    uint64_t bytes;  // of its values, in whole 16-byte units
};
inline uint64_t units(uint64_t len) { return (len + 15) & ~(uint64_t)15; }

// `layout` (ah_node_layout = legacy::Layout): which split values the passes read.  Under a legacy layout every Item child
// becomes a one-id Descendants node behind the nodes of the values, in the upgrade's order (node_legacy.h)
int create_from_encoded(ah_dataset *ds, int layout, const uint32_t *node_ids, const uint8_t *const *values, const size_t *lens, size_t n_nodes,
                        const uint32_t *root_ids, uint32_t n_trees, ah_index **out, ah_index_decode_stats *out_stats,
                        ah_index_legacy_stats *out_legacy) {
    using Clock = IndexCall::Clock;
    const auto t_begin = Clock::now();
    if (out_stats) *out_stats = ah_index_decode_stats{};
    if (out_legacy) *out_legacy = ah_index_legacy_stats{};
    AH_REQUIRE(out, AH_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    AH_REQUIRE(legacy::layout_valid(layout), AH_ERR_INVALID_ARGUMENT, "unknown node layout %d (AH_NODE_LAYOUT_V0_7, _V0_5, _V0_4)", layout);
    AH_REQUIRE(ds, AH_ERR_INVALID_ARGUMENT, "dataset is NULL");
    const bool old = layout != legacy::L_V0_7;
    AH_REQUIRE(n_nodes == 0 || (node_ids && values && lens), AH_ERR_INVALID_ARGUMENT, "%s is NULL", !node_ids ? "node_ids" : !values ? "values" : "lens");
    AH_REQUIRE(n_trees == 0 || root_ids, AH_ERR_INVALID_ARGUMENT, "root_ids is NULL");
    AH_REQUIRE(ds->finalized, AH_ERR_NOT_FINALIZED, "dataset not finalized");
    AH_REQUIRE(n_nodes < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT, "forest too large for 32-bit node / descendant offsets");
    uint64_t largest = 16;
    for (size_t i = 0; i < n_nodes; i++) {
        AH_REQUIRE(values[i], AH_ERR_INVALID_ARGUMENT, "node %u: values[%zu] is NULL", node_ids[i], i);
        AH_REQUIRE(i == 0 || node_ids[i - 1] < node_ids[i], AH_ERR_INVALID_ARGUMENT,
                   "node_ids is not strictly ascending at position %zu (node %u after node %u)", i, node_ids[i], node_ids[i - 1]);
        AH_REQUIRE(lens[i] <= 0x7FFFFFFFull, AH_ERR_INVALID_ARGUMENT, "node %u: a value of %zu bytes", node_ids[i], lens[i]);
        largest = std::max(largest, units(lens[i]));
    }
    // the chunks, from the lengths alone
    const uint64_t chunk_bytes = std::max<uint64_t>(largest, (uint64_t)std::max<long long>(0, tun(TUN_DECODE_CHUNK_BYTES)));
    std::vector<Chunk> chunks;
    uint64_t max_values = 0, max_staging = 0;
    for (size_t i = 0; i < n_nodes;) {
        Chunk c{i, i, 0};
        while (c.hi < n_nodes && c.bytes + units(lens[c.hi]) <= chunk_bytes) c.bytes += units(lens[c.hi++]);
        max_values = std::max<uint64_t>(max_values, c.hi - c.lo);
        max_staging = std::max<uint64_t>(max_staging, (c.hi - c.lo) * sizeof(DecValue) + c.bytes);
        chunks.push_back(c);
        i = c.hi;
    }
    IndexCall call;
    AH_TRY(call.begin(ds));
    const hipStream_t s = call.stream();
    const uint32_t nn = (uint32_t)n_nodes;
    const uint32_t hs = (uint32_t)ah_header_size(ds->metric), vs = (uint32_t)ah_vector_size(ds->metric, ds->dims);
    const uint32_t hf = header_floats(ds->metric);
    const size_t row_bytes = ds->row_bytes();
    // every block but those that grow with what the values hold: [ctl][cnt][nrm][info][tile sums] and the staging; a legacy
    // layout adds [itm][the chunk's Item ids, two per value] behind the tile sums
    const size_t ctl_bytes = (sizeof(DecCtl) + 15) & ~(size_t)15, per = (size_t)((max_values * 4 + 15) & ~(uint64_t)15);
    const size_t sums_bytes = (size_t)((((max_values + kScanTile - 1) / kScanTile + 1) * 4 + 15) & ~(uint64_t)15);
    DevMem d_ids, nodes, roots, work, staging, desc, nrows, nhdrs, items;
    AH_TRY(alloc(&d_ids, (size_t)nn * 4));
    AH_TRY(alloc(&nodes, std::max<size_t>(1, nn) * sizeof(DNode)));
    AH_TRY(alloc(&roots, std::max<size_t>(1, n_trees) * 4));
    AH_TRY(alloc(&work, ctl_bytes + 3 * per + sums_bytes + (old ? 3 * per : 0)));
    AH_TRY(alloc(&staging, (size_t)max_staging));
    AH_TRY(call.lease->c->ensure_pinned((size_t)std::max<uint64_t>(max_staging, 16)));
    uint8_t *pin = reinterpret_cast<uint8_t *>(call.lease->c->h_pinned);
    DecCtl *d_ctl = work.as<DecCtl>();
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(work.as<uint8_t>() + ctl_bytes);
    uint32_t *d_nrm = reinterpret_cast<uint32_t *>(work.as<uint8_t>() + ctl_bytes + per);
    uint32_t *d_info = reinterpret_cast<uint32_t *>(work.as<uint8_t>() + ctl_bytes + 2 * per);
    uint32_t *d_sums = reinterpret_cast<uint32_t *>(work.as<uint8_t>() + ctl_bytes + 3 * per);
    uint32_t *d_itm = old ? reinterpret_cast<uint32_t *>(work.as<uint8_t>() + ctl_bytes + 3 * per + sums_bytes) : nullptr;
    uint32_t *d_new = old ? reinterpret_cast<uint32_t *>(work.as<uint8_t>() + ctl_bytes + 4 * per + sums_bytes) : nullptr;
    auto clear_ctl = [&]() -> int {
        AH_HIP(hipMemsetAsync(d_ctl, 0, sizeof(DecCtl), s));
        AH_HIP(hipMemsetAsync(&d_ctl->w[DW_ERR], 0xFF, 8, s));
        return AH_OK;
    };
    auto refused = [&](unsigned long long err, bool root) -> int {
        const uint32_t at = (uint32_t)(err >> 8), reason = (uint32_t)(err & 0xFF);
        if (root) AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "root %u (node %u): %s", at, root_ids[at], decode::reason_text(reason));
        AH_REQUIRE(false, AH_ERR_INVALID_ARGUMENT, "node %u (position %u): %s", node_ids[at], at, legacy::reason_text(reason));
        return AH_OK;
    };
    ah_index_decode_stats st{};
    st.values = n_nodes;
    DecCtl ctl{};
    if (nn) AH_HIP(hipMemcpyAsync(d_ids.p, node_ids, (size_t)nn * 4, hipMemcpyHostToDevice, s));
    if (n_trees) {
        AH_HIP(hipMemcpyAsync(roots.p, root_ids, (size_t)n_trees * 4, hipMemcpyHostToDevice, s));
        AH_TRY(clear_ctl());
        hipLaunchKernelGGL(k_dec_roots, dim3(grid_of(n_trees, kDecBlock, 1024)), dim3(kDecBlock), 0, s, roots.as<uint32_t>(), n_trees,
                           d_ids.as<const uint32_t>(), nn, d_ctl);
        AH_TRY(read_back(&ctl, d_ctl, 2, s));
        if (ctl.w[DW_ERR] != ~0ull) return refused(ctl.w[DW_ERR], true);
    }
    uint64_t desc_cap = 0, nrows_cap = 0, nhdrs_cap = 0, items_cap = 0, ids_total = 0, normals_total = 0, leaves = 0, items_total = 0, zeros = 0;
    const uint32_t f32 = metric_is_bq(ds->metric) ? 0u : 1u;
    const uint64_t span = call.span();
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        const Chunk &c = chunks[ci];
        const bool last = ci + 1 == chunks.size();
        const uint32_t n = (uint32_t)(c.hi - c.lo);
        // the copy: descriptors, then every value at a 16-byte boundary with zeroes behind it.  The host reads no byte of a value
        const auto t_copy = Clock::now();
        const uint64_t values_at = (uint64_t)n * sizeof(DecValue);
        DecValue *h_vals = reinterpret_cast<DecValue *>(pin);
        uint64_t at = values_at;
        for (size_t i = c.lo; i < c.hi; i++) {
            h_vals[i - c.lo] = DecValue{(uint32_t)i, (uint32_t)lens[i], at};
            if (lens[i]) memcpy(pin + at, values[i], lens[i]);
            const uint64_t u = units(lens[i]);
            if (u != lens[i]) memset(pin + at + lens[i], 0, (size_t)(u - lens[i]));
            at += u;
        }
        st.seconds_host_copy += IndexCall::secs(t_copy, Clock::now());
        st.bytes_staged += at;
        st.chunks++;
        const DecValue *d_vals = staging.as<const DecValue>();
        const uint8_t *d_staging = staging.as<const uint8_t>();
        AH_TRY(clear_ctl());
        AH_HIP(hipMemcpyAsync(staging.p, pin, (size_t)at, hipMemcpyHostToDevice, s));
        for_spans(n, span, [&](uint64_t lo, uint64_t hi) {
            hipLaunchKernelGGL(k_dec_measure, dim3(grid_of(hi - lo, kDecBlock / kWave, 4096)), dim3(kDecBlock), 0, s, d_staging, d_vals, (uint32_t)lo,
                               (uint32_t)(hi - lo), layout, f32, hs, vs, nodes.as<DNode>(), d_cnt, d_nrm, d_info, d_itm, d_ctl);
        });
        launch_exclusive_scan(d_cnt, n, d_sums, &d_ctl->ids_total, s);
        launch_exclusive_scan(d_nrm, n, d_sums, &d_ctl->normals_total, s);
        if (old) launch_exclusive_scan(d_itm, n, d_sums, &d_ctl->items_total, s);
        hipLaunchKernelGGL(k_dec_links, dim3(grid_of(n, kDecBlock, 4096)), dim3(kDecBlock), 0, s, d_vals, n, d_ids.as<const uint32_t>(), nn,
                           nodes.as<DNode>(), (const uint32_t *)d_cnt, (const uint32_t *)d_nrm, (const uint32_t *)d_itm, (uint32_t)ids_total,
                           (uint32_t)normals_total, (uint32_t)items_total, d_new, d_ctl);
        AH_TRY(read_back(&ctl, d_ctl, sizeof(DecCtl) / 4, s));
        const uint64_t items_now = items_total + ctl.w[DW_ITEMS];  // the new nodes so far: each a node slot and one id
        AH_REQUIRE(n_nodes + items_now < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT,
                   "node %u: the split values up to it have %llu Item children, each a new node: forest too large for 32-bit node / descendant offsets",
                   node_ids[c.hi - 1], (unsigned long long)items_now);
        AH_REQUIRE(ids_total + ctl.w[DW_IDS] + items_now < 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT,
                   "node %u: the Descendants values up to it hold %llu ids: forest too large for 32-bit node / descendant offsets", node_ids[c.hi - 1],
                   (unsigned long long)(ids_total + ctl.w[DW_IDS] + items_now));
        AH_REQUIRE(ctl.ids_total == ctl.w[DW_IDS] && ctl.normals_total == ctl.w[DW_NORMALS] && (!old || ctl.items_total == ctl.w[DW_ITEMS]),
                   AH_ERR_DEVICE, "the scans of the decode lost count");
        // Room for what the chunk holds (the last chunk leaves every array at its exact size), then the payloads.  A chunk with a
        // refused value is expanded all the same — a refused value is no node and holds no id — so that a container at fault in
        // a value before it is the one named: the smallest position of the call
        AH_TRY(fit(&desc, &desc_cap, ids_total * 4, (ids_total + ctl.w[DW_IDS] + (last ? items_now : 0)) * 4, last, s));
        if (ctl.w[DW_ITEMS]) {  // the chunk's Item ids behind those of the chunks before
            AH_TRY(fit(&items, &items_cap, items_total * 4, items_now * 4, false, s));
            AH_HIP(hipMemcpyAsync(items.as<uint32_t>() + items_total, d_new, (size_t)ctl.w[DW_ITEMS] * 4, hipMemcpyDeviceToDevice, s));
        }
        const uint64_t rows = normals_total + ctl.w[DW_NORMALS], rows_room = std::max<uint64_t>(1, rows);
        AH_TRY(fit(&nrows, &nrows_cap, normals_total * row_bytes, rows_room * row_bytes, last, s));
        AH_TRY(fit(&nhdrs, &nhdrs_cap, normals_total * hf * 4, rows_room * hf * 4, last, s));
        for_spans(n, span, [&](uint64_t lo, uint64_t hi) {
            const uint32_t first = (uint32_t)lo, m = (uint32_t)(hi - lo);
            if (ctl.w[DW_NORMALS])
                hipLaunchKernelGGL(k_dec_normals, dim3(grid_of(m, kDecBlock / kWave, 8192)), dim3(kDecBlock), 0, s, d_staging, d_vals, first, m,
                                   nodes.as<const DNode>(), old ? legacy::kSplitHead : codec::kSplitHead, old ? 0u : hs, old ? 0u : hf, vs / 4,
                                   (uint32_t)(row_bytes / 4), (uint32_t)rows, nrows.as<uint32_t>(), nhdrs.as<float>());
            if (ctl.w[DW_WAVE_VALUES])
                hipLaunchKernelGGL(k_dec_desc_wave, dim3(grid_of(m, kDecBlock / kWave, 4096)), dim3(kDecBlock), 0, s, d_staging, d_vals, first, m,
                                   nodes.as<const DNode>(), (const uint32_t *)d_info, desc.as<uint32_t>(), ids_total + ctl.w[DW_IDS], d_ctl);
            if (ctl.w[DW_BLOCK_VALUES])
                hipLaunchKernelGGL(k_dec_desc_block, dim3(grid_of(m, 1, 2048)), dim3(kDecBlock), 0, s, d_staging, d_vals, first, m,
                                   nodes.as<const DNode>(), (const uint32_t *)d_info, desc.as<uint32_t>(), ids_total + ctl.w[DW_IDS], d_ctl);
        });
        if (old && ctl.w[DW_NORMALS]) {  // `D::new_header` of the chunk's rows, by the kernel that makes the headers of uploaded vectors
            DataView dv = ds->view();
            dv.n = rows;
            dv.rows_f32 = f32 ? nrows.as<const float>() : nullptr;
            dv.rows_bq = f32 ? nullptr : nrows.as<const uint64_t>();
            dv.headers = nhdrs.as<float>();
            AH_TRY(launch_headers_from_vectors(dv, normals_total, ctl.w[DW_NORMALS], s));
        }
        unsigned long long err = ~0ull;
        AH_TRY(read_back(&err, &d_ctl->w[DW_ERR], 2, s));
        if (err != ~0ull) return refused(err, false);
        ids_total += ctl.w[DW_IDS];
        normals_total += ctl.w[DW_NORMALS];
        leaves += ctl.w[DW_LEAVES];
        items_total = items_now;
        zeros += ctl.w[DW_ZEROS];
        st.split_values += ctl.w[DW_SPLITS];
        st.containers_array += ctl.w[DW_ARRAYS], st.containers_bitmap += ctl.w[DW_BITMAPS], st.containers_run += ctl.w[DW_RUNS];
        st.wave_values += ctl.w[DW_WAVE_VALUES];
        st.block_containers += ctl.w[DW_BLOCK_CONTAINERS];
    }
    if (chunks.empty()) {
        AH_TRY(fit(&desc, &desc_cap, 0, 4, true, s));
        AH_TRY(fit(&nrows, &nrows_cap, 0, row_bytes, true, s));
        AH_TRY(fit(&nhdrs, &nhdrs_cap, 0, (uint64_t)hf * 4, true, s));
    }
    const uint32_t n_values = nn, n_new = (uint32_t)items_total;
    if (n_new) {  // the one-id nodes behind the nodes of the values, their ids behind the lists of the values
        uint64_t nodes_cap = (uint64_t)n_values * sizeof(DNode);
        AH_TRY(fit(&nodes, &nodes_cap, nodes_cap, (uint64_t)(n_values + n_new) * sizeof(DNode), true, s));
        hipLaunchKernelGGL(k_dec_new_nodes, dim3(grid_of(n_new, kDecBlock, 4096)), dim3(kDecBlock), 0, s, items.as<const uint32_t>(), n_new,
                           (uint32_t)ids_total, nodes.as<DNode>() + n_values, desc.as<uint32_t>() + ids_total);
        AH_HIP(hipGetLastError());
    }
    // what validate_forest_view asks of a view, on the node records as the index will hold them: every node reachable from at
    // most one root / parent (children and roots are ranks or new slots, hence in range; nodes no root reaches are legal)
    const uint32_t n_all = n_values + n_new;
    auto id_of = [&](uint32_t i) { return i < n_values ? node_ids[i] : node_ids[n_values - 1] + 1 + (i - n_values); };
    std::vector<DNode> h_nodes(n_all);
    std::vector<uint32_t> h_roots(n_trees);
    if (n_all) AH_HIP(hipMemcpyAsync(h_nodes.data(), nodes.p, (size_t)n_all * sizeof(DNode), hipMemcpyDeviceToHost, s));
    if (n_trees) AH_HIP(hipMemcpyAsync(h_roots.data(), roots.p, (size_t)n_trees * 4, hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    uint32_t max_desc = 0;
    for (uint32_t i = 0; i < n_all; i++)
        if (h_nodes[i].kind == AH_NODE_DESCENDANTS) max_desc = std::max(max_desc, h_nodes[i].b);
    {
        std::vector<uint8_t> seen(n_all, 0);
        std::vector<uint32_t> stack;
        for (uint32_t t = 0; t < n_trees; t++) {
            stack.push_back(h_roots[t]);
            while (!stack.empty()) {
                const uint32_t i = stack.back();
                stack.pop_back();
                AH_REQUIRE(i < n_all, AH_ERR_DEVICE, "the decode left a link out of range");
                AH_REQUIRE(!seen[i], AH_ERR_INVALID_ARGUMENT,
                           "node %u (position %u) is reachable twice (cycle or shared sub-tree): the values are not a forest", id_of(i), i);
                seen[i] = 1;
                if ((h_nodes[i].kind & 0xFFu) == AH_NODE_SPLIT) {
                    stack.push_back(h_nodes[i].a);
                    stack.push_back(h_nodes[i].b);
                }
            }
        }
    }
    // the index: nothing below can fail but the handle itself
    std::unique_ptr<ah_index> ix(new ah_index());
    NoFailScope no_fail;
    auto take = [](DevMem &m) {
        void *p = m.p;
        m.p = nullptr;
        return p;
    };
    ix->ds = ds;
    ix->n_trees = n_trees;
    ix->n_nodes = n_all;
    ix->desc_len = ids_total + n_new;
    ix->n_normals = (uint32_t)normals_total;
    ix->normals_cap = std::max<uint32_t>(1, ix->n_normals);
    ix->n_leaves = (uint32_t)leaves + n_new;
    ix->max_desc = max_desc;
    ix->compacted = true;
    ix->d_nodes = static_cast<DNode *>(take(nodes));
    ix->d_roots = static_cast<uint32_t *>(take(roots));
    ix->d_desc = static_cast<uint32_t *>(take(desc));
    ix->d_nrows = take(nrows);
    ix->d_nhdrs = static_cast<float *>(take(nhdrs));
    index_prepare_screens(ds);
    ix->nv.metric = ds->metric;
    ix->nv.dims = ds->dims;
    ix->nv.pitch = ds->pitch;
    ix->nv.words = ds->words;
    index_derive_normals_view(ix.get());
    ix->nv.ids = nullptr;
    ix->nv.lut = nullptr;
    ix->nv.lut_len = 0;
    ix->nv.identity_ids = 1;
    ds->live_indexes.fetch_add(1, std::memory_order_acq_rel);
    ix->counted = true;
    st.normals = normals_total;
    st.descendants_values = leaves;
    st.ids = ids_total;
    st.seconds_total = IndexCall::secs(t_begin, Clock::now());
    if (call.timing)
        fprintf(stderr, "[ah] index from encoded nodes: %zu values (%llu split, %llu with a normal, %llu Descendants of %llu ids) in %llu chunks, "
                        "%llu bytes staged: %.6f s, of them %.6f s the host copy\n",
                n_nodes, (unsigned long long)st.split_values, (unsigned long long)st.normals, (unsigned long long)st.descendants_values,
                (unsigned long long)st.ids, (unsigned long long)st.chunks, (unsigned long long)st.bytes_staged, st.seconds_total, st.seconds_host_copy);
    if (out_stats) *out_stats = st;
    if (out_legacy && old) *out_legacy = ah_index_legacy_stats{st.split_values, zeros, normals_total, items_total, items_total};
    *out = ix.release();
    return AH_OK;
}

}  // namespace
}  // namespace ah

extern "C" {

int ah_index_create_from_encoded(ah_dataset *ds, const uint32_t *node_ids, const uint8_t *const *values, const size_t *lens, size_t n_nodes,
                                 const uint32_t *root_ids, uint32_t n_trees, ah_index **out, ah_index_decode_stats *out_stats) {
    AH_GUARDED("ah_index_create_from_encoded")
    ah::DeviceRestore restore_device;
    return ah::create_from_encoded(ds, AH_NODE_LAYOUT_V0_7, node_ids, values, lens, n_nodes, root_ids, n_trees, out, out_stats, nullptr);
    AH_GUARDED_END
}

int ah_index_create_from_legacy(ah_dataset *ds, int layout, const uint32_t *node_ids, const uint8_t *const *values, const size_t *lens,
                                size_t n_nodes, const uint32_t *root_ids, uint32_t n_trees, ah_index **out, ah_index_decode_stats *out_stats,
                                ah_index_legacy_stats *out_legacy) {
    AH_GUARDED("ah_index_create_from_legacy")
    ah::DeviceRestore restore_device;
    return ah::create_from_encoded(ds, layout, node_ids, values, lens, n_nodes, root_ids, n_trees, out, out_stats, out_legacy);
    AH_GUARDED_END
}

}  // extern "C"
