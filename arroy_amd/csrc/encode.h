// Launchers of encode.hip: tree nodes -> the bytes LMDB stores (node_codec.h), many nodes per launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ah_dataset;

namespace ah {

// One node of an encode launch.  Descendants: its ids are the u32 at byte `src` of the launch's source, `a` of them.
// Split: its normal record starts at byte `src` of the source, `a` / `b` are the ids of its children.
struct EncNode {
    uint64_t src;
    uint32_t a, b;
};
static_assert(sizeof(EncNode) == 16, "uploaded as is");

constexpr uint32_t kEncErrOrder = 1u;   // error word: a list does not ascend strictly
constexpr uint32_t kEncHasBitmap = 2u;  // ... (no error) some list has a container of more than 4096 ids
constexpr uint32_t kEncScanTile = 1024; // lengths per block of the scan
inline size_t enc_scan_sums(uint64_t n) { return (size_t)((n + kEncScanTile - 1) / kEncScanTile + 1); }
// info words of a mixed sequence (index_encode.hip) for the nodes that are no Descendants nodes: the measure leaves their
// lengths as its caller wrote them, both Descendants writers skip them.  (A list has at most 65 536 containers.)
constexpr uint32_t kEncInfoSplit = 0xFFFFFFFFu, kEncInfoFree = 0xFFFFFFFEu;

// Measure + scan of `n` Descendants nodes, all on `s`: off[0 .. n] = exclusive 64-bit prefix sum of the value lengths
// (off[n]: the total), info[i] = container count | bit 31: the list has a bitmap container; *err gets kEncErr* bits OR-ed in
// (the caller zeroes it).  sums: enc_scan_sums(n) words of scratch.
int launch_measure_descendants(const uint8_t *src, const EncNode *nodes, uint64_t n, uint64_t *off, uint32_t *info, uint64_t *sums,
                               uint32_t *err, hipStream_t s);
// The same over a mixed sequence: the caller has written info[i] = kEncInfoSplit / kEncInfoFree and off[i] = the value length
// for every node that is no Descendants node, and info[i] = 0 for the others; one scan runs over all the lengths.
int launch_measure_mixed(const uint8_t *src, const EncNode *nodes, uint64_t n, uint64_t *off, uint32_t *info, uint64_t *sums,
                         uint32_t *err, hipStream_t s);
// Values of nodes [0, n) to out + off[i] - out_base.  any_bitmap: what the measure reported (the block-per-list kernel for
// lists with bitmap containers is launched only then).
int launch_write_descendants(const uint8_t *src, const EncNode *nodes, uint64_t n, const uint64_t *off, const uint32_t *info,
                             uint64_t out_base, uint8_t *out, bool any_bitmap, hipStream_t s);
// Split values: node i is off[i + 1] - off[i] bytes long — 9, or 9 + header_size + vector_size with the header at
// src + nodes[i].src + hdr_off and the vector at src + nodes[i].src.
int launch_write_splits(const uint8_t *src, const EncNode *nodes, uint64_t n, const uint64_t *off, uint64_t out_base, uint8_t *out,
                        uint32_t hdr_off, uint32_t header_size, hipStream_t s);

// ah_encode_descendants without the entry-point guard (the one-node trees of an encoded streaming build use it too)
int encode_id_lists(ah_dataset *ds, const uint32_t *ids, const uint64_t *offsets, size_t n_lists, uint8_t *out_values,
                    uint64_t out_cap, uint64_t *out_value_offsets);

}  // namespace ah
