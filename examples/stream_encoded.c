/* What the encoded node stream saves a Writer: the same streaming build with three sinks, one per run of this program.
 *
 *   stream_encoded host    [n dims trees repeats]   ah_build_forest_stream, the sink encodes every node on the calling host
 *                                                   thread (the encoder of examples/shim_roundtrip.c) into an arena
 *   stream_encoded encoded [n dims trees repeats]   ah_build_forest_stream_encoded, the sink copies the values into an arena
 *   stream_encoded empty   [n dims trees repeats]   ah_build_forest_stream, the sink looks at nothing (the build alone)
 *
 * Defaults: synthetic 1M x 768 cosine, 50 trees, one warm-up and five timed builds.  Prints one line per build and the
 * median; `host` and `encoded` also print the arena's length and a checksum, which must agree between the two (the
 * values are the same bytes; only their order of arrival inside the arena is the stream's).
 *
 * The encoded entry point is a v7 addition: it is looked up at run time, so the program also runs (modes `host` and
 * `empty`) against a library that does not have it yet.
 *
 *   cc -std=c99 -O2 -Iinclude examples/stream_encoded.c -Larroy_amd -larroy_hip -ldl -Wl,-rpath,$PWD/arroy_amd -o stream_encoded
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "arroy_hip.h"

typedef struct arena {
    uint8_t *bytes;
    size_t len, cap;
    size_t hs, vs;        /* D::Header / vector bytes */
    uint64_t nodes, sum;  /* values taken, sum over values of (id + 1) * (first byte + last byte + length) */
} arena;

static uint8_t *arena_take(arena *t, size_t n) {
    if (t->len + n > t->cap) {
        t->cap = 2 * (t->len + n) + 4096;
        t->bytes = (uint8_t *)realloc(t->bytes, t->cap);
        if (!t->bytes) return NULL;
    }
    uint8_t *p = t->bytes + t->len;
    t->len += n;
    return p;
}
static void account(arena *t, uint32_t id, const uint8_t *p, size_t n) {
    t->nodes++;
    t->sum += ((uint64_t)id + 1) * ((uint64_t)p[0] + p[n - 1] + n);
}
static void put_be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

/* RoaringBitmap::serialize_into for ascending u32 ids, as examples/shim_roundtrip.c writes it */
static int roaring_serialize(arena *t, const uint32_t *ids, size_t n) {
    size_t n_cont = 0;
    for (size_t i = 0; i < n; i++)
        if (i == 0 || (ids[i] >> 16) != (ids[i - 1] >> 16)) n_cont++;
    uint8_t *hdr = arena_take(t, 8 + 8 * n_cont);
    if (!hdr) return 1;
    const size_t hdr_at = (size_t)(hdr - t->bytes);
    const uint32_t cookie = 12346, nc = (uint32_t)n_cont;
    memcpy(hdr, &cookie, 4);
    memcpy(hdr + 4, &nc, 4);
    size_t c = 0, i = 0;
    uint32_t offset = (uint32_t)(8 + 8 * n_cont);
    while (i < n) {
        size_t j = i;
        while (j < n && (ids[j] >> 16) == (ids[i] >> 16)) j++;
        const size_t card = j - i;
        const uint16_t key = (uint16_t)(ids[i] >> 16), cm1 = (uint16_t)(card - 1);
        const size_t body = card <= 4096 ? 2 * card : 8192;
        uint8_t *out = arena_take(t, body);
        if (!out) return 1;
        hdr = t->bytes + hdr_at;
        memcpy(hdr + 8 + 4 * c, &key, 2);
        memcpy(hdr + 8 + 4 * c + 2, &cm1, 2);
        memcpy(hdr + 8 + 4 * n_cont + 4 * c, &offset, 4);
        if (card <= 4096) {
            for (size_t k = 0; k < card; k++) {
                const uint16_t low = (uint16_t)(ids[i + k] & 0xFFFFu);
                memcpy(out + 2 * k, &low, 2);
            }
        } else {
            memset(out, 0, 8192);
            for (size_t k = 0; k < card; k++) out[(ids[i + k] & 0xFFFFu) >> 3] |= (uint8_t)(1u << (ids[i + k] & 7u));
        }
        offset += (uint32_t)body;
        c++;
        i = j;
    }
    return 0;
}

/* (a) raw batches: encode every node here */
static int sink_host(void *user, const ah_node_batch *b) {
    arena *t = (arena *)user;
    for (uint64_t i = 0; i < b->n_nodes; i++) {
        const ah_stream_node *nd = &b->nodes[i];
        const size_t at = t->len;
        if (nd->kind == AH_NODE_SPLIT) {
            const size_t n = 9 + (nd->has_normal ? t->hs + t->vs : 0);
            uint8_t *p = arena_take(t, n);
            if (!p) return 1;
            p[0] = 2;
            put_be32(p + 1, nd->left);
            put_be32(p + 5, nd->right);
            if (nd->has_normal) {
                const uint8_t *rec = b->payload + nd->payload_offset;
                memcpy(p + 9, rec + b->normal_header_offset, t->hs);
                memcpy(p + 9 + t->hs, rec + b->normal_vector_offset, t->vs);
            }
        } else {
            uint8_t *p = arena_take(t, 1);
            if (!p) return 1;
            p[0] = 1;
            if (roaring_serialize(t, (const uint32_t *)(b->payload + nd->payload_offset), nd->count)) return 1;
        }
        account(t, nd->id, t->bytes + at, t->len - at);
    }
    return 0;
}
/* (b) encoded batches: the values are ready, copy them */
static int sink_encoded(void *user, const ah_node_batch *b) {
    arena *t = (arena *)user;
    if (b->normal_stride != 0) return 2; /* not an encoded batch */
    uint8_t *p = arena_take(t, (size_t)b->payload_len);
    if (!p) return 1;
    memcpy(p, b->payload, (size_t)b->payload_len);
    for (uint64_t i = 0; i < b->n_nodes; i++) {
        const uint64_t lo = b->nodes[i].payload_offset, hi = i + 1 < b->n_nodes ? b->nodes[i + 1].payload_offset : b->payload_len;
        account(t, b->nodes[i].id, p + lo, (size_t)(hi - lo));
    }
    return 0;
}
static int sink_empty(void *user, const ah_node_batch *b) {
    arena *t = (arena *)user;
    t->nodes += b->n_nodes;
    return 0;
}

static double now(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static int cmp_double(const void *a, const void *b) {
    const double x = *(const double *)a, y = *(const double *)b;
    return x < y ? -1 : x > y;
}
#define CHECK(expr)                                                                   \
    do {                                                                              \
        if ((expr) != AH_OK) {                                                        \
            fprintf(stderr, "%s failed: %s\n", #expr, ah_last_error());               \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s host|encoded|empty [n dims trees repeats]\n", argv[0]);
        return 2;
    }
    const char *mode = argv[1];
    const uint64_t n = argc > 2 ? strtoull(argv[2], NULL, 10) : 1000000;
    const uint32_t dims = argc > 3 ? (uint32_t)strtoul(argv[3], NULL, 10) : 768;
    const uint32_t trees = argc > 4 ? (uint32_t)strtoul(argv[4], NULL, 10) : 50;
    const int repeats = argc > 5 ? atoi(argv[5]) : 5;
    const int encoded = strcmp(mode, "encoded") == 0, host = strcmp(mode, "host") == 0;
    if (!encoded && !host && strcmp(mode, "empty") != 0) return 2;
    if (repeats < 1 || repeats > 64) return 2;

    typedef int (*build_encoded_fn)(ah_dataset *, const ah_build_options *, const ah_encode_options *, ah_node_batch_fn, void *,
                                    uint32_t *, ah_build_stats *);
    build_encoded_fn build_encoded = NULL;
    *(void **)&build_encoded = dlsym(RTLD_DEFAULT, "ah_build_forest_stream_encoded");
    if (encoded && !build_encoded) {
        fprintf(stderr, "this libarroy_hip has no ah_build_forest_stream_encoded\n");
        return 3;
    }
    ah_dataset *ds = NULL;
    CHECK(ah_dataset_create(AH_COSINE, dims, n, 0, &ds));
    CHECK(ah_dataset_fill_synthetic(ds, 42, 1, n));
    CHECK(ah_dataset_finalize(ds));
    uint64_t *seeds = (uint64_t *)malloc(sizeof(uint64_t) * trees);
    uint32_t *roots = (uint32_t *)malloc(sizeof(uint32_t) * trees);
    if (!seeds || !roots) return 1;
    for (uint32_t t = 0; t < trees; t++) seeds[t] = 1000 + t;
    ah_build_options opt;
    memset(&opt, 0, sizeof opt);
    opt.n_trees = trees;
    opt.tree_seeds = seeds;
    ah_encode_options enc = {0, 0};
    arena t;
    memset(&t, 0, sizeof t);
    t.hs = ah_header_size(AH_COSINE);
    t.vs = ah_vector_size(AH_COSINE, dims);
    double took[64];
    for (int r = -1; r < repeats; r++) { /* r == -1: the warm-up */
        t.len = 0;
        t.nodes = t.sum = 0;
        ah_build_stats st;
        const double t0 = now();
        if (encoded) CHECK(build_encoded(ds, &opt, &enc, sink_encoded, &t, roots, &st));
        else CHECK(ah_build_forest_stream(ds, &opt, host ? sink_host : sink_empty, &t, roots, &st));
        const double dt = now() - t0;
        if (r >= 0) took[r] = dt;
        printf("%s %s: %.4f s (device %.4f s), %llu nodes, %zu bytes, checksum %llu\n", mode, r < 0 ? "warm-up" : "build", dt,
               st.seconds_device, (unsigned long long)t.nodes, t.len, (unsigned long long)t.sum);
    }
    qsort(took, (size_t)repeats, sizeof(double), cmp_double);
    printf("%s median %.4f s, min %.4f s, max %.4f s over %d builds of %llu x %u, %u trees\n", mode, took[repeats / 2], took[0],
           took[repeats - 1], repeats, (unsigned long long)n, dims, trees);
    free(t.bytes);
    free(seeds);
    free(roots);
    CHECK(ah_dataset_destroy(ds));
    return 0;
}
