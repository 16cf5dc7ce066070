// Tree nodes -> the bytes LMDB stores for them (node_codec.h), on the device: a segmented, variable-length encode.
//
//   measure   one wavefront per id list: container boundaries (a change of id >> 16 between neighbours), container count,
//             value length, strict ascent
//   scan      64-bit exclusive prefix sum of the lengths over any number of lists (tile sums, one block over the sums, apply)
//   write     Descendants: one wavefront per list when every container is an array (the rule: a list of at most 4096 ids
//             always is); one block per list otherwise — containers one after the other, a bitmap zeroed and OR-ed in LDS.
//             Split values: one wavefront per node, [2][BE left][BE right][header][vector] out of the level's record table.
//
// Values lie back to back, so most start at odd addresses: every store is a byte store, except the aligned 4-byte spans
// of a split value's body.  No kernel reads what another thread wrote to global memory.
#include "common.h"
#include "encode.h"
#include "node_codec.h"

namespace ah {
namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kEncBlock = 256;

struct ChunkScan {  // what one 64-id step of a list knows about container boundaries
    uint64_t mask;  // lanes whose id starts a container
    uint32_t cur;
    bool valid, boundary, bad;
};
__device__ __forceinline__ ChunkScan scan_step(const uint32_t *ids, uint32_t count, uint32_t base, uint32_t lane) {
    ChunkScan r;
    const uint32_t i = base + lane;
    r.valid = i < count;
    r.cur = r.valid ? ids[i] : 0u;
    const uint32_t prev = (r.valid && i) ? ids[i - 1] : 0u;
    r.boundary = r.valid && (i == 0 || (r.cur >> 16) != (prev >> 16));
    r.bad = r.valid && i && r.cur <= prev;
    r.mask = __ballot(r.boundary);
    return r;
}

// A container that is still open when a 64-id step ends is closed by the first boundary of a later step (or by the end of
// the list); one that starts and ends inside a step has at most 64 ids.  So only the carried one can be a bitmap.
__global__ __launch_bounds__(kEncBlock) void k_enc_measure(const uint8_t *__restrict__ src, const EncNode *__restrict__ nodes, uint64_t n,
                                                          uint64_t *__restrict__ len_out, uint32_t *__restrict__ info,
                                                          uint32_t *__restrict__ err, bool mixed) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t n_waves = (uint64_t)gridDim.x * (kEncBlock / kWave);
    for (uint64_t node = ((uint64_t)blockIdx.x * kEncBlock + threadIdx.x) / kWave; node < n; node += n_waves) {
        if (mixed && info[node] >= kEncInfoFree) continue;  // no Descendants node: its length is its caller's
        const EncNode nd = nodes[node];
        const uint32_t *ids = reinterpret_cast<const uint32_t *>(src + nd.src);
        const uint32_t count = nd.a;
        uint32_t nc = 0, open_i = 0;
        uint64_t saved = 0;  // bytes the bitmap containers take less than 2 per id
        bool bad = false;
        for (uint32_t base = 0; base < count; base += kWave) {
            const ChunkScan c = scan_step(ids, count, base, lane);
            bad = bad || c.bad;
            if (c.mask) {
                if (nc) {
                    const uint32_t card = base + (uint32_t)__ffsll((long long)c.mask) - 1 - open_i;
                    if (card > codec::kArrayMax) saved += 2ull * card - codec::kBitmapBytes;
                }
                open_i = base + 63 - (uint32_t)__clzll((long long)c.mask);
                nc += (uint32_t)__popcll(c.mask);
            }
        }
        if (nc && count - open_i > codec::kArrayMax) saved += 2ull * (count - open_i) - codec::kBitmapBytes;
        const bool any_bad = __ballot(bad) != 0;
        if (lane == 0) {
            len_out[node] = codec::descendants_value_len(nc, 2ull * count - saved);
            info[node] = nc | (saved ? 0x80000000u : 0u);
            const uint32_t flags = (any_bad ? kEncErrOrder : 0u) | (saved ? kEncHasBitmap : 0u);
            if (flags) atomicOr(err, flags);
        }
    }
}

// ---- scan: v[0, n) lengths -> exclusive prefix sums in place, v[n] = total -------------------------------------------------
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t x, uint64_t *sh, uint64_t *total) {
    const uint32_t t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (uint32_t d = 1; d < kEncBlock; d <<= 1) {
        const uint64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[kEncBlock - 1];
    __syncthreads();
    return incl - x;
}
__global__ __launch_bounds__(kEncBlock) void k_enc_scan_sums(const uint64_t *__restrict__ v, uint64_t n, uint64_t *__restrict__ sums) {
    __shared__ uint64_t sh[kEncBlock];
    const uint64_t lo = (uint64_t)blockIdx.x * kEncScanTile + (uint64_t)threadIdx.x * 4;
    uint64_t x = 0;
    for (uint32_t u = 0; u < 4; u++)
        if (lo + u < n) x += v[lo + u];
    uint64_t total;
    (void)block_exclusive_scan(x, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one block: sums[0, nb) -> exclusive, sums[nb] = v[n] = the grand total
__global__ __launch_bounds__(kEncBlock) void k_enc_scan_top(uint64_t *__restrict__ sums, uint64_t nb, uint64_t *__restrict__ v, uint64_t n) {
    __shared__ uint64_t sh[kEncBlock];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nb; base += kEncBlock) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t x = i < nb ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan(x, sh, &total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        sums[nb] = carry;
        v[n] = carry;
    }
}
__global__ __launch_bounds__(kEncBlock) void k_enc_scan_apply(uint64_t *__restrict__ v, uint64_t n, const uint64_t *__restrict__ sums) {
    __shared__ uint64_t sh[kEncBlock];
    const uint64_t lo = (uint64_t)blockIdx.x * kEncScanTile + (uint64_t)threadIdx.x * 4;
    uint64_t x[4], mine = 0;
    for (uint32_t u = 0; u < 4; u++) {
        x[u] = lo + u < n ? v[lo + u] : 0;
        mine += x[u];
    }
    uint64_t total;
    uint64_t at = sums[blockIdx.x] + block_exclusive_scan(mine, sh, &total);
    for (uint32_t u = 0; u < 4; u++) {
        if (lo + u < n) v[lo + u] = at;
        at += x[u];
    }
}

// ---- Descendants, every container an array: the low 16 bits of id i lie at 8 + 8 nc + 2 i -----------------------------------
__global__ __launch_bounds__(kEncBlock) void k_enc_write_desc(const uint8_t *__restrict__ src, const EncNode *__restrict__ nodes, uint64_t n,
                                                             const uint64_t *__restrict__ off, const uint32_t *__restrict__ info,
                                                             uint64_t out_base, uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t n_waves = (uint64_t)gridDim.x * (kEncBlock / kWave);
    for (uint64_t node = ((uint64_t)blockIdx.x * kEncBlock + threadIdx.x) / kWave; node < n; node += n_waves) {
        const uint32_t nc = info[node];
        if (nc >> 31) continue;  // k_enc_write_desc_big's
        const EncNode nd = nodes[node];
        const uint32_t *ids = reinterpret_cast<const uint32_t *>(src + nd.src);
        const uint32_t count = nd.a;
        uint8_t *tag = out + (off[node] - out_base);
        uint8_t *v = tag + 1;
        if (lane == 0) {
            tag[0] = codec::kTagDescendants;
            codec::put_le32(v, codec::kRoaringCookie);
            codec::put_le32(v + 4, nc);
        }
        uint8_t *pairs = v + 8, *offs = v + 8 + 4ull * nc;
        const uint32_t body = 8 + 8 * nc;
        uint32_t seen = 0, open_i = 0, open_c = 0;
        for (uint32_t base = 0; base < count; base += kWave) {
            const ChunkScan c = scan_step(ids, count, base, lane);
            const uint32_t i = base + lane;
            if (c.valid) codec::put_le16(v + body + 2ull * i, c.cur & 0xFFFFu);
            if (c.mask) {
                if (seen && lane == 0)
                    codec::put_le16(pairs + 4ull * open_c + 2, base + (uint32_t)__ffsll((long long)c.mask) - 1 - open_i - 1);
                if (c.boundary) {
                    const uint32_t k = seen + (uint32_t)__popcll(c.mask & ((1ull << lane) - 1));
                    codec::put_le16(pairs + 4ull * k, c.cur >> 16);
                    codec::put_le32(offs + 4ull * k, body + 2 * i);
                    const uint64_t after = lane == kWave - 1 ? 0ull : c.mask >> (lane + 1);
                    if (after) codec::put_le16(pairs + 4ull * k + 2, (uint32_t)__ffsll((long long)after) - 1);  // cardinality - 1
                }
                const uint32_t here = (uint32_t)__popcll(c.mask);
                open_i = base + 63 - (uint32_t)__clzll((long long)c.mask);
                open_c = seen + here - 1;
                seen += here;
            }
        }
        if (seen && lane == 0) codec::put_le16(pairs + 4ull * open_c + 2, count - open_i - 1);
    }
}

// ---- Descendants with bitmap containers: one block per list, container after container ---------------------------------------
__global__ __launch_bounds__(kEncBlock) void k_enc_write_desc_big(const uint8_t *__restrict__ src, const EncNode *__restrict__ nodes, uint64_t n,
                                                                 const uint64_t *__restrict__ off, const uint32_t *__restrict__ info,
                                                                 uint64_t out_base, uint8_t *__restrict__ out) {
    __shared__ uint32_t bits[codec::kBitmapBytes / 4];
    const uint32_t t = threadIdx.x;
    for (uint64_t node = blockIdx.x; node < n; node += gridDim.x) {
        const uint32_t inf = info[node];
        if (!(inf >> 31) || inf >= kEncInfoFree) continue;
        const uint32_t nc = inf & 0x7FFFFFFFu;
        const EncNode nd = nodes[node];
        const uint32_t *ids = reinterpret_cast<const uint32_t *>(src + nd.src);
        const uint32_t count = nd.a;
        uint8_t *tag = out + (off[node] - out_base);
        uint8_t *v = tag + 1;
        if (t == 0) {
            tag[0] = codec::kTagDescendants;
            codec::put_le32(v, codec::kRoaringCookie);
            codec::put_le32(v + 4, nc);
        }
        uint64_t at = 8 + 8ull * nc;
        uint32_t i = 0;
        for (uint32_t c = 0; i < count && c < nc; c++) {
            const uint32_t key = ids[i] >> 16;
            uint32_t lo = i + 1, hi = count;  // the ids ascend: the container ends at the first larger key
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if ((ids[mid] >> 16) == key) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t card = lo - i;
            if (t == 0) {
                codec::put_le16(v + 8 + 4ull * c, key);
                codec::put_le16(v + 8 + 4ull * c + 2, card - 1);
                codec::put_le32(v + 8 + 4ull * nc + 4ull * c, (uint32_t)at);
            }
            if (card <= codec::kArrayMax) {
                for (uint32_t k = t; k < card; k += kEncBlock) codec::put_le16(v + at + 2ull * k, ids[i + k] & 0xFFFFu);
            } else {
                for (uint32_t w = t; w < codec::kBitmapBytes / 4; w += kEncBlock) bits[w] = 0;
                __syncthreads();
                for (uint32_t k = t; k < card; k += kEncBlock) {
                    const uint32_t low = ids[i + k] & 0xFFFFu;  // bit low & 7 of byte low >> 3 = bit low & 31 of LE word low >> 5
                    atomicOr(&bits[low >> 5], 1u << (low & 31u));
                }
                __syncthreads();
                for (uint32_t b = t; b < codec::kBitmapBytes; b += kEncBlock) v[at + b] = (uint8_t)(bits[b >> 2] >> (8 * (b & 3u)));
                __syncthreads();
            }
            at += codec::container_body_len(card);
            i = lo;
        }
    }
}

// ---- split values ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEncBlock) void k_enc_write_split(const uint8_t *__restrict__ src, const EncNode *__restrict__ nodes, uint64_t n,
                                                              const uint64_t *__restrict__ off, uint64_t out_base, uint8_t *__restrict__ out,
                                                              uint32_t hdr_off, uint32_t header_size) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t n_waves = (uint64_t)gridDim.x * (kEncBlock / kWave);
    for (uint64_t node = ((uint64_t)blockIdx.x * kEncBlock + threadIdx.x) / kWave; node < n; node += n_waves) {
        const EncNode nd = nodes[node];
        const uint64_t begin = off[node];
        const uint32_t len = (uint32_t)(off[node + 1] - begin);
        uint8_t *dst = out + (begin - out_base);
        const uint8_t *vec = src + nd.src, *hdr = vec + hdr_off;
        auto byte_at = [&](uint32_t j) { return (uint32_t)codec::split_value_byte(j, nd.a, nd.b, hdr, header_size, vec); };
        // bytes up to the first 4-byte boundary of the destination, aligned words, bytes again
        const uint32_t head = min(len, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
        const uint32_t words = (len - head) / 4;
        if (lane < head) dst[lane] = (uint8_t)byte_at(lane);
        for (uint32_t w = lane; w < words; w += kWave) {
            const uint32_t j = head + 4 * w;
            *reinterpret_cast<uint32_t *>(dst + j) = byte_at(j) | byte_at(j + 1) << 8 | byte_at(j + 2) << 16 | byte_at(j + 3) << 24;
        }
        const uint32_t j = head + 4 * words + lane;
        if (j < len) dst[j] = (uint8_t)byte_at(j);
    }
}

unsigned wave_grid(uint64_t n) { return grid_of(n, kEncBlock / kWave, 256u * 16u); }

}  // namespace

static int measure_and_scan(const uint8_t *src, const EncNode *nodes, uint64_t n, uint64_t *off, uint32_t *info, uint64_t *sums, uint32_t *err,
                            bool mixed, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_enc_measure, dim3(wave_grid(n)), dim3(kEncBlock), 0, s, src, nodes, n, off, info, err, mixed);
    const uint64_t nb = (n + kEncScanTile - 1) / kEncScanTile;
    if (nb) hipLaunchKernelGGL(k_enc_scan_sums, dim3((unsigned)nb), dim3(kEncBlock), 0, s, off, n, sums);
    hipLaunchKernelGGL(k_enc_scan_top, dim3(1), dim3(kEncBlock), 0, s, sums, nb, off, n);
    if (nb) hipLaunchKernelGGL(k_enc_scan_apply, dim3((unsigned)nb), dim3(kEncBlock), 0, s, off, n, sums);
    AH_HIP(hipGetLastError());
    return AH_OK;
}

int launch_measure_descendants(const uint8_t *src, const EncNode *nodes, uint64_t n, uint64_t *off, uint32_t *info, uint64_t *sums,
                               uint32_t *err, hipStream_t s) {
    return measure_and_scan(src, nodes, n, off, info, sums, err, false, s);
}

int launch_measure_mixed(const uint8_t *src, const EncNode *nodes, uint64_t n, uint64_t *off, uint32_t *info, uint64_t *sums, uint32_t *err,
                         hipStream_t s) {
    return measure_and_scan(src, nodes, n, off, info, sums, err, true, s);
}

int launch_write_descendants(const uint8_t *src, const EncNode *nodes, uint64_t n, const uint64_t *off, const uint32_t *info,
                             uint64_t out_base, uint8_t *out, bool any_bitmap, hipStream_t s) {
    if (!n) return AH_OK;
    hipLaunchKernelGGL(k_enc_write_desc, dim3(wave_grid(n)), dim3(kEncBlock), 0, s, src, nodes, n, off, info, out_base, out);
    if (any_bitmap)
        hipLaunchKernelGGL(k_enc_write_desc_big, dim3(grid_of(n, 1, 1024u)), dim3(kEncBlock), 0, s, src, nodes, n, off, info, out_base, out);
    AH_HIP(hipGetLastError());
    return AH_OK;
}

int launch_write_splits(const uint8_t *src, const EncNode *nodes, uint64_t n, const uint64_t *off, uint64_t out_base, uint8_t *out,
                        uint32_t hdr_off, uint32_t header_size, hipStream_t s) {
    if (!n) return AH_OK;
    hipLaunchKernelGGL(k_enc_write_split, dim3(wave_grid(n)), dim3(kEncBlock), 0, s, src, nodes, n, off, out_base, out, hdr_off, header_size);
    AH_HIP(hipGetLastError());
    return AH_OK;
}

int encode_id_lists(ah_dataset *ds, const uint32_t *ids, const uint64_t *offsets, size_t n_lists, uint8_t *out_values, uint64_t out_cap,
                    uint64_t *out_value_offsets) {
    AH_REQUIRE(ds && offsets && out_value_offsets, AH_ERR_INVALID_ARGUMENT, "NULL argument");
    for (size_t i = 0; i < n_lists; i++)
        AH_REQUIRE(offsets[i + 1] >= offsets[i] && offsets[i + 1] - offsets[i] <= 0xFFFFFFFFull, AH_ERR_INVALID_ARGUMENT,
                   "offsets must be non-decreasing, a list holds at most 2^32 - 1 ids");
    const uint64_t total_ids = offsets[n_lists] - offsets[0];
    AH_REQUIRE(ids || total_ids == 0, AH_ERR_INVALID_ARGUMENT, "ids is NULL");
    out_value_offsets[0] = 0;
    if (n_lists == 0) return AH_OK;
    AH_HIP(hipSetDevice(ds->device));
    ContextLease lease(ds);
    AH_REQUIRE(lease.c, AH_ERR_DEVICE, "cannot create a HIP stream");
    hipStream_t s = lease.c->stream;
    std::vector<EncNode> nodes(n_lists);
    for (size_t i = 0; i < n_lists; i++) nodes[i] = EncNode{(offsets[i] - offsets[0]) * 4, (uint32_t)(offsets[i + 1] - offsets[i]), 0u};
    DevMem d_ids, d_nodes, d_off, d_info, d_sums, d_err, d_out;
    AH_TRY(alloc(&d_ids, total_ids * 4, "the id lists"));
    AH_TRY(alloc(&d_nodes, n_lists * sizeof(EncNode), "the id lists"));
    AH_TRY(alloc(&d_off, (n_lists + 1) * 8, "the value offsets"));
    AH_TRY(alloc(&d_info, n_lists * 4, "the value offsets"));
    AH_TRY(alloc(&d_sums, enc_scan_sums(n_lists) * 8, "the value offsets"));
    AH_TRY(alloc(&d_err, 4, "the value offsets"));
    if (total_ids) AH_HIP(hipMemcpyAsync(d_ids.p, ids + offsets[0], total_ids * 4, hipMemcpyHostToDevice, s));
    AH_HIP(hipMemcpyAsync(d_nodes.p, nodes.data(), n_lists * sizeof(EncNode), hipMemcpyHostToDevice, s));
    AH_HIP(hipMemsetAsync(d_err.p, 0, 4, s));
    AH_TRY(launch_measure_descendants(d_ids.as<uint8_t>(), d_nodes.as<EncNode>(), n_lists, d_off.as<uint64_t>(), d_info.as<uint32_t>(),
                                      d_sums.as<uint64_t>(), d_err.as<uint32_t>(), s));
    uint32_t err = 0;
    AH_HIP(hipMemcpyAsync(out_value_offsets, d_off.p, (n_lists + 1) * 8, hipMemcpyDeviceToHost, s));
    AH_HIP(hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    AH_REQUIRE(!(err & kEncErrOrder), AH_ERR_INVALID_ARGUMENT, "id lists must be strictly ascending (RoaringBitmap order)");
    if (!out_values) return AH_OK;
    const uint64_t total = out_value_offsets[n_lists];
    AH_REQUIRE(total <= out_cap, AH_ERR_INVALID_ARGUMENT, "the values need %llu bytes, out_cap is %llu", (unsigned long long)total,
               (unsigned long long)out_cap);
    AH_TRY(alloc(&d_out, total, "the encoded values"));
    AH_TRY(launch_write_descendants(d_ids.as<uint8_t>(), d_nodes.as<EncNode>(), n_lists, d_off.as<uint64_t>(), d_info.as<uint32_t>(), 0,
                                    d_out.as<uint8_t>(), (err & kEncHasBitmap) != 0, s));
    AH_HIP(hipMemcpyAsync(out_values, d_out.p, total, hipMemcpyDeviceToHost, s));
    AH_HIP(hipStreamSynchronize(s));
    return AH_OK;
}

}  // namespace ah

extern "C" {

int ah_encode_descendants(ah_dataset *ds, const uint32_t *ids, const uint64_t *offsets, size_t n_lists, uint8_t *out_values,
                          uint64_t out_cap, uint64_t *out_value_offsets) {
    AH_GUARDED("ah_encode_descendants")
    return ah::encode_id_lists(ds, ids, offsets, n_lists, out_values, out_cap, out_value_offsets);
    AH_GUARDED_END
}

}  // extern "C"
