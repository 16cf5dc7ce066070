/* The plain-C host encoder of examples/stream_encoded.c (roaring_serialize into its arena, one tag byte in front of every
 * value) over id lists the caller holds, for scripts/measure_index_encode.py.  The example is included as it is, its main
 * renamed by the compile line (-Dmain=stream_encoded_main). */
#include "../examples/stream_encoded.c"

#if defined(__GNUC__)
#define MIE_EXPORT __attribute__((visibility("default")))
#else
#define MIE_EXPORT
#endif

/* lists[i] = ids[offsets[i] .. offsets[i + 1]); returns 0 and the bytes written and the seconds taken, arena included */
MIE_EXPORT int host_encode_lists(const uint32_t *ids, const uint64_t *offsets, size_t n_lists, uint64_t *out_bytes, double *out_seconds) {
    arena t;
    memset(&t, 0, sizeof t);
    const double t0 = now();
    for (size_t i = 0; i < n_lists; i++) {
        uint8_t *tag = arena_take(&t, 1);
        if (!tag) return 1;
        *tag = 1;
        if (roaring_serialize(&t, ids + offsets[i], (size_t)(offsets[i + 1] - offsets[i]))) return 1;
    }
    *out_seconds = now() - t0;
    *out_bytes = t.len;
    free(t.bytes);
    return 0;
}
