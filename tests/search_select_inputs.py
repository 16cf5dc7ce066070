"""Designed inputs for the selections of ah_search_batch (arroy_amd/csrc/search.hip: k_search_select, and
k_search_select_screened with and without the de-duplication fused into it), shared by test_search_select_cpu.py (which proves
on the CPU that every input has the property it is named for) and test_gpu_search_select.py (which runs them).

Exact distances.  Rows of 32 dims (the narrowest the leaf tiles take) are (c, 0, ..., 0).  DotProduct: a query (s, 1, 0, ...)
with s a power of two is at distance -(s * c) bit for bit, so a case chooses every distance word (`dot_case`: c = -f32(word),
s = 1, 2, 4 ... move every word by whole exponents and keep their offsets).  Euclidean: the query (0, 2^-20, 0, ...) is at
c * c + 2^-40 = c * c in f32 for |c| >= 1, exact for c = (2048 + j) / 2048 (12 significant bits), so a case chooses among
those values and the ties between them.

Exact candidate sets.  Every tree holds ONE chosen list of ids (`views`: a root plane over the list and an empty list), and
search_k is the number of listed ids: a query's candidates are the union of the lists, with every id repeated as often as trees
hold it.  Every query carries a second component that only the root planes see (the rows are zero there).  Ids are the
rows' positions (the LDS bitmap flags the duplicates: the fused selection of a call of few queries can run) or sparse, the last
one beyond 39 * 1024 * 32 (the bitmap does not fit: k_flag_duplicates_hash and the non-fused selections).

`selection` restates the bins of the kernels from their comments — 2048 bins over the span of the ordered words, direct when
the span is <= 2048, else scale = floor(2048 * 2^32 / span); the bin of the k-th key; the keys up to that bin — and is used
ONLY to classify an input as served or left to the sorted path.  Expected answers come from numpy on the chosen distances
(`Case.expect`) and from the oracle.

Screened inputs (`screened_case`) need no model of the error bounds: group A is m copies of one vector under m ids (equal
screen values, equal bounds: they survive or fall together), every other row points the opposite way (cosine ~2 against ~0,
dot at least +|v|^2 / 2 against -|v|^2: tens of thousands of bins above any threshold).  `clustered` is the near-tie cluster
test_gpu_query_screens.py imports from here, whose behaviour against the same bounds is established there for the re-rank."""
import ctypes as C

import numpy as np

DIMS = 32
BINS, CAP = 2048, 1024
BITMAP_IDS = 39 * 1024 * 32     # ids the LDS bitmap of the de-duplication covers
W_ONE = 0xBF800000              # ordered word of 1.0f
SHAPES = (1, 8, 32, 70)         # queries a call: fused selection / own units / k_units_small / past the small kernels
TREES = 9                       # two blocks of k_descend_multi


def ordered_words(d):
    """OrderedFloat<f32> as an unsigned word: NaN greatest and all NaNs equal, -0 == +0."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    b = d.view(np.uint32).astype(np.uint64)
    w = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    w[d == 0] = 0x80000000
    w[np.isnan(d)] = 0xFFFFFFFF
    return w


def f32_of_words(w):
    """the inverse of ordered_words for finite, non-zero distances"""
    w = np.asarray(w, dtype=np.uint64)
    b = np.where(w & 0x80000000, w & 0x7FFFFFFF, ~w & 0xFFFFFFFF)
    return b.astype(np.uint32).view(np.float32)


# ---- the restatement, for classification only --------------------------------------------------------------------------------

def bins_of(words, w_min, span):
    words = np.asarray(words, dtype=np.uint64)
    if span <= BINS:
        return (words - np.uint64(w_min)).astype(np.int64), 0
    scale = (BINS << 32) // span  # (< 2^32, as the offsets are: the products fit 64 bits)
    return (((words - np.uint64(w_min)) * np.uint64(scale)) >> np.uint64(32)).astype(np.int64), scale


def t_key_closed(w_min, w_max, span, scale, bin_k):
    """The largest word of bin `bin_k` as the screened selection computes it (the closed form next to `t_key`)."""
    if span <= BINS:
        return w_min + bin_k
    lim = (bin_k + 1) << 32
    d = (lim + scale - 1) // scale
    return min(w_min + d - 1, w_max)


def selection(words, k):
    """What k_search_select computes before it sorts, for the ordered words of a query's DISTINCT candidates and k = count."""
    words = np.asarray(words, dtype=np.uint64)
    kk = min(k, len(words))
    if kk == 0:
        return {"kk": 0, "n_sel": 0, "served": True}
    w_min, w_max = int(words.min()), int(words.max())
    span = w_max - w_min + 1
    bins, scale = bins_of(words, w_min, span)
    hist = np.bincount(bins, minlength=BINS)
    assert len(hist) == BINS
    upto = np.cumsum(hist)
    bin_k = int(np.searchsorted(upto, kk))          # the first bin with upto >= kk
    kth = int(np.sort(words)[kk - 1])
    t_key = t_key_closed(w_min, w_max, span, scale, bin_k)
    first = w_min + bin_k if span <= BINS else w_min + -(-(bin_k << 32) // scale)
    return {"kk": kk, "span": span, "direct": span <= BINS, "scale": scale, "bin_k": bin_k, "n_sel": int(upto[bin_k]),
            "served": int(upto[bin_k]) <= CAP, "kth": kth, "bin_first": first, "bin_last": t_key, "w_min": w_min}


# ---- forests of single Descendants roots -------------------------------------------------------------------------------------

def spread(ids, n_trees=TREES, per=7):
    """`n_trees` lists: id number i is in the trees t with (i - t) mod n_trees < per — every id `per` times"""
    ids = np.asarray(ids, dtype=np.uint32)
    pos = np.arange(len(ids))
    return [ids[(pos - t) % n_trees < per] for t in range(n_trees)]


def views(trees, metric, dims=DIMS):
    """-> (view for ah_index_create_from_view, the same for the oracle, keep-alive, listed ids).  Tree t: a split root
    (node 3t + 2) over the list (node 3t) and an empty list (node 3t + 1).  Its normal is (0, t + 1, 0, ...) with a zero header,
    so the margins of a query whose second component is not zero differ from tree to tree: roots that were Descendants nodes
    themselves would all carry the key +inf, and the block descents of a small call leave equal keys of two trees to the
    sequential descent (`fallback_queue`).  With search_k = the listed ids every list is read whatever the order."""
    from arroy_amd import _lib
    from arroy_amd.dataset import _NODE_DT
    from oracle import oracle as O
    hs, vs = (8 if metric == O.DOT_PRODUCT else 4), 4 * dims
    nodes = np.zeros(3 * len(trees), dtype=_NODE_DT)
    normals = np.zeros((len(trees), (hs + vs) // 4), dtype=np.float32)
    at = 0
    for t, ids in enumerate(trees):
        assert np.all(np.diff(np.asarray(ids, dtype=np.int64)) > 0)
        nodes["kind"][3 * t], nodes["offset"][3 * t], nodes["count"][3 * t] = 1, at, len(ids)
        at += len(ids)
        nodes["kind"][3 * t + 1], nodes["offset"][3 * t + 1] = 1, at
        nodes["kind"][3 * t + 2], nodes["has_normal"][3 * t + 2], nodes["offset"][3 * t + 2] = 2, 1, t * (hs + vs)
        nodes["left"][3 * t + 2], nodes["right"][3 * t + 2] = 3 * t, 3 * t + 1
        normals[t, hs // 4 + 1] = t + 1
    desc = np.concatenate(trees).astype(np.uint32)
    roots = (3 * np.arange(len(trees)) + 2).astype(np.uint32)
    blob = normals.view(np.uint8).reshape(-1)
    out = []
    for mod, node_t in ((_lib, _lib.AhNode), (O, O.AhNode)):
        v = mod.AhForestView()
        v.n_trees, v.n_nodes = len(trees), len(nodes)
        v.roots = roots.ctypes.data_as(C.POINTER(C.c_uint32))
        v.nodes = C.cast(nodes.ctypes.data, C.POINTER(node_t))
        v.normals = blob.ctypes.data_as(C.POINTER(C.c_uint8))
        v.normals_len = blob.size
        v.normal_stride, v.normal_vector_offset, v.normal_header_offset = hs + vs, hs, 0
        v.descendants = desc.ctypes.data_as(C.POINTER(C.c_uint32))
        v.descendants_len = len(desc)
        out.append(v)
    return out[0], out[1], (nodes, desc, roots, blob, normals), len(desc)


def sparse_ids(n):
    """n ascending ids, unequal to the rows' positions, the last one beyond what the LDS bitmap covers"""
    step = BITMAP_IDS // (n - 1) + 2
    ids = (np.arange(n, dtype=np.uint64) * step + 5).astype(np.uint32)
    assert ids[-1] >= BITMAP_IDS
    return ids


# ---- cases of exact distances --------------------------------------------------------------------------------------------------

class Case:
    """Rows (c, 0, ...) in `vectors`, the rows listed by the trees in `listed` (positions; the others are stored and in no
    tree: a filter may name them), `count`, an optional filter (positions) and what the selection must do with it."""

    def __init__(self, name, metric, c, listed, count, served, same_ids=False, keep=None, n_sel=None):
        self.name, self.metric, self.count, self.served, self.n_sel = name, metric, count, served, n_sel
        self.c = np.asarray(c, dtype=np.float32)
        self.listed = np.asarray(listed, dtype=np.int64)
        self.same_ids, self.keep = same_ids, None if keep is None else np.asarray(keep, dtype=np.int64)
        self.vectors = np.zeros((len(self.c), DIMS), dtype=np.float32)
        self.vectors[:, 0] = self.c
        assert 9 * len(self.listed) <= 16384 if same_ids else 7 * len(self.listed) <= 16384  # (the fused selection's limit)

    def ids(self, sparse):
        return sparse_ids(len(self.c)) if sparse else np.arange(len(self.c), dtype=np.uint32)

    def trees(self, sparse, n_trees=TREES, per=7):
        ids = self.ids(sparse)[self.listed]
        return [ids] * n_trees if self.same_ids else spread(ids, n_trees, per)

    def queries(self, nq):
        q = np.zeros((nq, DIMS), dtype=np.float32)
        q[:, 1] = 1.0 if self.metric == "dot" else 2.0 ** -20  # (seen by the root planes only)
        if self.metric == "dot":
            q[:, 0] = [2.0 ** (i % 4) for i in range(nq)]
        return q

    def distances(self, q):
        """the reference's distance of every row from query q, chosen bit for bit"""
        return -(q[0] * self.c) if self.metric == "dot" else self.c * self.c

    def candidates(self):
        """positions of the distinct candidates of every query"""
        return self.listed if self.keep is None else np.intersect1d(self.listed, self.keep)

    def words(self, q):
        return ordered_words(self.distances(q)[self.candidates()])

    def expect(self, q, sparse, count=None):
        """(ids, normalized distances: -d for DotProduct, the root for Euclidean) by a plain sort of (ordered word, id)"""
        pos = self.candidates()
        d = self.distances(q)[pos]
        ids = self.ids(sparse)[pos]
        order = np.lexsort((ids, ordered_words(d)))[: self.count if count is None else count]
        return ids[order], (-d[order] if self.metric == "dot" else np.sqrt(d[order]))


def dot_case(name, offsets, count, served, extra=200, **kw):
    """DotProduct rows whose distances from (1, 0, ...) are the words W_ONE + offsets; `extra` rows more in no tree"""
    off = np.asarray(offsets, dtype=np.uint64)
    d = f32_of_words(np.uint64(W_ONE) + off)
    rng = np.random.default_rng(len(off))
    d = d[rng.permutation(len(d))]  # (ids in no order of the distances)
    c = np.concatenate([-d, np.full(extra, -1.5, dtype=np.float32)])
    return Case(name, "dot", c, np.arange(len(off)), count, served, **kw)


def euclid_c(j):
    return ((2048 + np.asarray(j, dtype=np.int64)) / 2048.0).astype(np.float32)


def euclid_case(name, c, count, served, extra=200, **kw):
    c = np.asarray(c, dtype=np.float32)
    rng = np.random.default_rng(len(c))
    c = c[rng.permutation(len(c))]
    return Case(name, "euclid", np.concatenate([c, np.full(extra, 1.5, dtype=np.float32)]), np.arange(len(c)), count, served, **kw)


def span_with_bin_width(width):
    """the smallest span beyond 2048 * (width - 1) whose bin 0 holds exactly `width` words"""
    span = BINS * (width - 1) + 1
    while True:
        scale = (BINS << 32) // span
        if -(-(1 << 32) // scale) == width:
            return span
        span += 1


def far(n, first, last):
    """n offsets from `first` to `last`, both taken"""
    return np.unique(np.linspace(first, last, n).astype(np.uint64))


def ties(m, b, hi, lo=None):
    """m distinct words, b keys on the next word, 1100 words beyond from offset `lo` (the very next word) to `hi`"""
    return np.concatenate([np.arange(m), np.full(b, m), far(1100, m + 1 if lo is None else lo, hi)])


def capacity_cases():
    """The unscreened selection at its capacity.  n_sel 1024 is served and 1025 is not, reached by equal distances around the
    k-th place and by distinct distances in the k-th key's bin, over direct and scaled spans."""
    w1024 = BINS * 1024              # scale = 2^22: every bin holds exactly 1024 words
    w1025 = span_with_bin_width(1025)
    assert (BINS << 32) // w1024 == 1 << 22 and w1025 == w1024 + 1
    out = [
        # equal distances around the k-th place: 500 distinct keys, 524 / 525 on one word, 1100 beyond
        dot_case("ties-direct-1024", ties(500, 524, 2047), 600, True, n_sel=1024),          # span 2048: the largest direct one
        dot_case("ties-direct-1025", ties(500, 525, 2047), 600, False, n_sel=1025),
        dot_case("ties-span2049-1024", ties(500, 524, 2048), 600, True, n_sel=1024),        # the smallest scaled span
        dot_case("ties-span2049-1025", ties(500, 525, 2048), 600, False, n_sel=1025),
        dot_case("ties-scaled-1024", ties(500, 524, 1 << 22, 4096), 501, True, n_sel=1024),       # k-th = the first of the equal keys
        dot_case("ties-scaled-1025", ties(500, 525, 1 << 22, 4096), 1024, False, n_sel=1025),     # k-th = the last but one
        # distinct distances, bins of exactly 1024 words: the k-th key on the LAST word of bin 0 ...
        dot_case("crowded-last-word-1024", np.concatenate([np.arange(1024), far(1100, 1024, w1024 - 1)]), 1024, True, n_sel=1024),
        # ... and on the FIRST word of bin 1, with 25 keys in bin 0 and 999 / 1000 in bin 1
        dot_case("crowded-first-word-1024", np.concatenate([[0], np.arange(1000, 1024), np.arange(1024, 2023),
                                                            far(1100, 2048, w1024 - 1)]), 26, True, n_sel=1024),
        dot_case("crowded-first-word-1025", np.concatenate([[0], np.arange(1000, 1024), np.arange(1024, 2024),
                                                            far(1100, 2048, w1024 - 1)]), 26, False, n_sel=1025),
        # bins of 1025 words, all of bin 0 taken
        dot_case("crowded-1025", np.concatenate([np.arange(1025), far(1100, 1025, w1025 - 1)]), 10, False, n_sel=1025),
        # fewer distinct candidates than count; the same ids in every tree (9 x 700 candidates, 700 distinct)
        dot_case("unique-below-count", np.arange(700) * 2, 1000, True, same_ids=True, n_sel=700),
        dot_case("same-ids-1024", np.concatenate([np.arange(1024), far(700, 5000, w1024 - 1)]), 10, True, same_ids=True, n_sel=1024),
        dot_case("same-ids-1025", np.concatenate([np.arange(1025), far(700, 5000, w1025 - 1)]), 10, False, same_ids=True, n_sel=1025),
        # the Euclidean twin: every distance equal (span 1: direct), and equal distances around the k-th place of a scaled span
        euclid_case("euclid-equal-1024", np.full(1024, 3.0), 100, True, same_ids=True, n_sel=1024),
        euclid_case("euclid-equal-1025", np.full(1025, 3.0), 100, False, same_ids=True, n_sel=1025),
        euclid_case("euclid-ties-1024", np.concatenate([euclid_c(np.arange(200)), np.full(824, euclid_c(300)),
                                                         4096 * euclid_c(np.arange(1100))]), 500, True, n_sel=1024),
        euclid_case("euclid-ties-1025", np.concatenate([euclid_c(np.arange(200)), np.full(825, euclid_c(300)),
                                                         4096 * euclid_c(np.arange(1100))]), 500, False, n_sel=1025),
    ]
    # filters over the rows of "ties-direct-1025": one that keeps nothing the trees list (kk == 0), one that keeps exactly
    # `count` listed rows (and some unlisted ones) — 600 of 2125, which leaves 600 distinct candidates
    base = out[1]
    n_listed = len(base.listed)
    unlisted = np.arange(n_listed, len(base.c))
    out.append(Case("filter-keeps-nothing", "dot", base.c, base.listed, 600, True, keep=unlisted, n_sel=0))
    kept = np.concatenate([np.arange(0, n_listed, 4)[:520], np.arange(1, n_listed, 4)[:80], unlisted[:50]])
    out.append(Case("filter-keeps-count", "dot", base.c, base.listed, 600, True, keep=np.sort(kept), n_sel=600))
    return out


def big_count_case():
    """2200 distinct candidates for `count` from 1024 to 2048: 1024 fits the selection on a direct span of 1024 words + far keys"""
    return dot_case("count-1024-to-2048", np.concatenate([np.arange(1024), far(1176, 4096, 1 << 21)]), 1024, True, n_sel=1024)


BIG_COUNTS = (1024, 1025, 1500, 2048)


# ---- screened inputs -------------------------------------------------------------------------------------------------------------

def screened_case(m, n_far=1100, seed=3):
    """-> (vectors, positions of group A, query base): group A = m copies of v at scattered positions, the others -v + noise
    at lengths from 0.5 to 1.5 (seen from -v their dot products lie far enough apart for a screen to tell them apart)"""
    rng = np.random.default_rng(seed)
    n = m + n_far
    v = rng.standard_normal(DIMS).astype(np.float32)
    vecs = (-v[None, :] * (0.5 + rng.random((n, 1))) + 0.05 * rng.standard_normal((n, DIMS))).astype(np.float32)
    a = np.sort(rng.choice(n, m, replace=False))
    vecs[a] = v
    return vecs, a, v


def screened_queries(v, nq, seed=5):
    rng = np.random.default_rng(seed)
    q = (v[None, :] + 0.02 * rng.standard_normal((nq, DIMS))).astype(np.float32)
    q[0] = v
    return q


def clustered(rng, n_far, n_near, dims, spread_):
    """n_near rows around a centre within `spread_`, n_far unrelated ones (the draws in this order: test_gpu_query_screens.py
    has established on the GPU how its seeds behave against the bounds)"""
    centre = rng.standard_normal(dims).astype(np.float32)
    near = centre + (rng.standard_normal((n_near, dims)) * spread_).astype(np.float32)
    far_ = rng.standard_normal((n_far, dims)).astype(np.float32)
    return np.concatenate([near, far_]).astype(np.float32), centre
