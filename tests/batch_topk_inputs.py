"""Designed inputs for the batched top-k of ah_rerank_batch (arroy_amd/csrc/batch.hip), shared by test_batch_topk_cpu.py
(which proves on the CPU that every input has the property it is named for) and test_gpu_batch_topk.py (which runs them),
and for the single-query top-k of ah_rerank_by_vector / _by_item (arroy_amd/csrc/distance.hip: k_topk_small, the tournament
and the global bitonic sort), shared by test_single_topk_cpu.py and test_gpu_single_topk.py in the same way.

The device that makes the inputs exact: a Manhattan dataset of 32 dims whose rows are (c, 0, ..., 0) and an all-zero query,
so that the distance of a row is |c| bit for bit and a test chooses every distance word.  Candidate lists are ascending in
id, hence in row: a list's distance sequence is laid out as a block of consecutive rows (`Blocks`).

Two restatements live here, written from the comments and constants of batch.hip and used ONLY to classify inputs ("this
query must be left to the tournament", "this list takes 4 rounds"), never as an expected answer:
  `tour_rounds`   chunks of 4096 keys, each block keeps min(k, 2048), the last block keeps k;
  `selection`     2048 bins over the span of the distance words (direct when the span is <= 2048, else
                  scale = floor(2048 * 2^32 / span)), the bin of the k-th key, and the count of keys up to that bin.
  `single_path`   the same bins without a sentinel word, and the limits of topk_small_fits (distance.hip): which of the three
                  single-query paths answers a list.
The expected answers come from `topk` (numpy, possible because the distances are chosen) and from the oracle."""
import numpy as np

DIMS = 32
MAX_ID = 0xFFFFFFFF
F32_MAX = np.float32(np.finfo(np.float32).max)
MAX_WORD = 0xFF7FFFFF           # ordered word of f32::MAX
CHUNK, SEL_BINS, SEL_CAP = 4096, 2048, 1024


def f32(words):
    return np.asarray(words, dtype=np.uint32).view(np.float32)


def word_of(x):
    return int(np.float32(x).view(np.uint32))


def ordered_words(d):
    """OrderedFloat<f32> as an unsigned word: NaN greatest and all NaNs equal, -0 == +0."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    b = d.view(np.uint32).astype(np.uint64)
    w = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    w[d == 0] = 0x80000000
    w[np.isnan(d)] = 0xFFFFFFFF
    return w


def skipped(d, ids, k, rule="reference"):
    """Which positions median_based_top_k (src/reader.rs:607-640) never looks at.  Its first 2k items are buffered unchecked.
    After them an item >= (f32::MAX, u32::MAX) is skipped while the threshold still has that initial value, that is until the
    first item below it arrives at a position >= 2k: that one compacts the buffer, the threshold becomes the k-th smallest
    key so far, and skipping against such a threshold changes no answer.
    rule: "reference" (the above), "every" (every such item from position 2k on), "none" (a plain sort)."""
    n = len(d)
    k = min(k, n)
    w = ordered_words(d)
    pos = np.arange(n)
    big = (w > MAX_WORD) | ((w == MAX_WORD) & (np.asarray(ids, dtype=np.uint64) == MAX_ID))
    beyond = pos >= 2 * k
    if rule == "none":
        return np.zeros(n, dtype=bool)
    if rule == "every":
        return big & beyond
    assert rule == "reference"
    below = np.flatnonzero(beyond & ~big)
    end = below[0] if below.size else n
    return big & beyond & (pos < end)


def topk(d, ids, k, rule="reference"):
    """(ids, normalized Manhattan distances) of the min(k, n) smallest (OrderedFloat word, position) keys."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.uint32)
    n = len(d)
    kk = min(k, n)
    keep = np.flatnonzero(~skipped(d, ids, k, rule))
    keys = (ordered_words(d)[keep] << np.uint64(32)) | keep.astype(np.uint64)
    pos = (np.sort(keys)[:kk] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert len(pos) == kk
    return ids[pos], np.fmax(d[pos], np.float32(0.0))  # Manhattan::normalized_distance is d.max(0.0): a NaN becomes 0


def canonical_bits(a):
    """f32 bits with every NaN as 0x7FC00000 (the view tests/test_gpu_query_screens.py uses): the sign and payload of a NaN
    that arithmetic produced are the platform's, not the algorithm's."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


# ---- restatements of batch.hip's design, for classification only -------------------------------------------------

def tour_rounds(n, k):
    """Rounds of the tournament for a list of n candidates and k = min(count, n) > 0."""
    rounds, n_in = 0, n
    while True:
        blocks = -(-n_in // CHUNK)
        keep = k if blocks == 1 else min(k, CHUNK // 2)
        n_in = blocks * keep
        rounds += 1
        if blocks == 1:
            return rounds


def final_buffer(n, k):
    """Round r writes buffer A when r is even, B when odd; the emit kernel reads what round `rounds - 1` wrote."""
    return "AB"[(tour_rounds(n, k) - 1) & 1]


def selection(d, ids, k, rule="reference"):
    """What k_batch_topk_select computes before it sorts: span, direct / scaled, the k-th key's bin, n_sel, flagged.
    rule="none": the bins of k_topk_small (distance.hip), which has no sentinel word."""
    n = len(d)
    kk = min(k, n)
    w = ordered_words(d)
    w[skipped(d, ids, k, rule)] = 0xFFFFFFFF      # a skipped key is the sentinel, whose word takes part in the span
    w_min, w_max = int(w.min()), int(w.max())
    span = w_max - w_min + 1
    direct = span <= SEL_BINS
    if direct:
        bins = (w - np.uint64(w_min)).astype(np.int64)
    else:
        scale = (SEL_BINS << 32) // span
        bins = np.array([((int(x) - w_min) * scale) >> 32 for x in w], dtype=np.int64)
    assert bins.min() >= 0 and bins.max() < SEL_BINS
    cum = np.cumsum(np.bincount(bins, minlength=SEL_BINS))
    bin_k = int(np.searchsorted(cum, kk))   # first bin whose running count reaches k
    n_sel = int(cum[bin_k])
    return {"span": span, "direct": direct, "bin": bin_k, "n_sel": n_sel, "flagged": n_sel > SEL_CAP}


SMALL_MAX_N, SMALL_MAX_K, BITONIC_K = 16384, 1024, CHUNK // 2


def single_path(d, ids, k):
    """Which path of distance.hip answers Dataset.rerank(k, ...) of this list with the defaults, and why:
    ("small", sel)          k_topk_small serves it; sel = its bins (no key is a sentinel there: any word above f32::MAX's
                            makes it decline, and with finite words only a skip could not change the answer);
    ("tournament", why) /
    ("bitonic", why)        the general path, chosen by k alone: k <= 2048 or not.  why = "limits" (topk_small_fits says no:
                            the kernel is not launched), "bit2" (a non-finite distance) or "bit3" (more than 1024 keys up to
                            the k-th key's bin).
    With AH_RERANK_SMALL=0 every list takes the general path."""
    n = len(d)
    kk = min(k, n)
    general = "tournament" if kk <= BITONIC_K else "bitonic"
    if not (n <= SMALL_MAX_N and kk <= SMALL_MAX_K and kk > 0):
        return general, "limits"
    if int(ordered_words(d).max()) > MAX_WORD:
        return general, "bit2"
    sel = selection(d, ids, kk, rule="none")
    return (general, "bit3") if sel["flagged"] else ("small", sel)


# ---- rows, ids, lists ------------------------------------------------------------------------------------

def sparse_ids(n):
    """Ascending, not the identity and not dense: position != id != row."""
    return (7 + 3 * np.arange(n, dtype=np.uint64) + (np.arange(n, dtype=np.uint64) // 5)).astype(np.uint32)


def vectors(c):
    """(c, 0, ..., 0) rows; finite values get alternating signs (|c| is the distance either way)."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    v = np.zeros((len(c), DIMS), dtype=np.float32)
    sign = np.where((np.arange(len(c)) & 1) == 1, np.float32(-1.0), np.float32(1.0))
    v[:, 0] = np.where(np.isfinite(c), c * sign, c)
    return v


class Blocks:
    """One block of consecutive rows per distance sequence.  `with_max_id`: the indices of the sequences whose list also
    ends with the dataset's last row, the item with id 0xFFFFFFFF, which holds f32::MAX."""

    def __init__(self, seqs, names=None, with_max_id=()):
        self.names = list(names) if names is not None else [str(i) for i in range(len(seqs))]
        seqs = [np.ascontiguousarray(s, dtype=np.float32) for s in seqs]
        total = sum(len(s) for s in seqs)
        has_last = len(with_max_id) > 0
        self.c = np.concatenate(seqs + ([np.array([F32_MAX], np.float32)] if has_last else []))
        self.ids = sparse_ids(len(self.c))
        if has_last:
            self.ids[-1] = MAX_ID
        self.rows, at = [], 0
        for i, s in enumerate(seqs):
            r = np.arange(at, at + len(s), dtype=np.uint32)
            if i in with_max_id:
                r = np.append(r, np.uint32(total))
            self.rows.append(r)
            at += len(s)
        self.vectors = vectors(self.c)
        self.query = np.zeros(DIMS, dtype=np.float32)

    def __len__(self):
        return len(self.rows)

    def index(self, name):
        return self.names.index(name)

    def dist(self, i):
        return np.abs(self.c[self.rows[i]])

    def list_ids(self, i):
        return self.ids[self.rows[i]]

    def expect(self, i, k, rule="reference"):
        return topk(self.dist(i), self.list_ids(i), k, rule)

    def select(self, i, k):
        return selection(self.dist(i), self.list_ids(i), k)

    def path(self, i, k):
        return single_path(self.dist(i), self.list_ids(i), k)


def subset_blocks(blocks, row_lists, names=None):
    """Lists that are ascending subsets of one dataset's rows instead of its blocks."""
    b = Blocks.__new__(Blocks)
    b.c, b.ids, b.vectors, b.query = blocks.c, blocks.ids, blocks.vectors, blocks.query
    b.rows = [np.ascontiguousarray(r, dtype=np.uint32) for r in row_lists]
    b.names = list(names) if names is not None else [str(len(r)) for r in b.rows]
    return b


ZERO_ID = 3   # below every id of sparse_ids


def with_zero_row(blocks):
    """The same lists on a dataset that has one more row in front, (0, ..., 0) under id ZERO_ID: re-ranking by that item is
    re-ranking by the all-zero query."""
    b = subset_blocks(blocks, [r + np.uint32(1) for r in blocks.rows], blocks.names)
    b.c = np.concatenate([np.zeros(1, np.float32), blocks.c])
    b.ids = np.concatenate([np.array([ZERO_ID], np.uint32), blocks.ids])
    assert b.ids[0] < b.ids[1]
    b.vectors = vectors(b.c)
    return b


def own_dataset(blocks, i, ids=None):
    """List i as a dataset of its own, whose "all items" is that list."""
    b = Blocks.__new__(Blocks)
    b.c, b.ids = blocks.c[blocks.rows[i]].copy(), (blocks.list_ids(i).copy() if ids is None else np.asarray(ids, np.uint32))
    b.vectors, b.query = vectors(b.c), blocks.query
    b.rows, b.names = [np.arange(len(b.c), dtype=np.uint32)], [blocks.names[i]]
    return b


# ---- case 1 and 6: 40 000 distinct distances ---------------------------------------------------------------

ROUNDS_N = (1, 100, 2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193, 9000, 20000, 40000, 0)
ROUNDS_K = (2048, 1025, 100, 1)


def distinct_rows(n=40000):
    rng = np.random.default_rng(1)
    return Blocks([f32(word_of(1.0) + rng.permutation(n).astype(np.uint32))])


def rounds_case():
    base = distinct_rows()
    rng = np.random.default_rng(2)
    n_rows = len(base.c)
    return subset_blocks(base, [np.sort(rng.choice(n_rows, n, replace=False)) for n in ROUNDS_N])


# ---- single query: the limits of the one-launch kernel, and the global sort ------------------------------------------

LIMITS = ((1, 1), (1023, 1023), (1024, 1024), (1025, 1024), (15361, 7), (16383, 1024), (16384, 1024), (16384, 1025),
          (16385, 1024), (16385, 1), (5, 10))


def limits_case():
    """One list of distinct distances per (n, k) of LIMITS, named `<n>-<k>`.  Every list of two or more holds the dataset's
    smallest and largest word, so all share one span (40 000 words, scaled bins of 19 or 20 words).  With k = 1024 < n a
    random list would put several keys after the k-th into its bin and overflow the kernel's 1024 slots, so those lists are
    drawn as 1024 rows from the bins up to one bin and n - 1024 rows from the bins after it: exactly 1024 selected keys."""
    base = distinct_rows()
    rng = np.random.default_rng(10)
    w = ordered_words(np.abs(base.c)).astype(np.int64)
    n_rows, lo, hi = len(w), int(np.argmin(w)), int(np.argmax(w))
    span = int(w[hi] - w[lo]) + 1
    bins = ((w - w[lo]) * ((SEL_BINS << 32) // span)) >> 32
    edge = int(np.searchsorted(np.cumsum(np.bincount(bins, minlength=SEL_BINS)), 4 * SEL_CAP))
    below, above = np.flatnonzero((bins <= edge) & (np.arange(n_rows) != lo)), np.flatnonzero((bins > edge) & (np.arange(n_rows) != hi))
    lists = []
    for n, k in LIMITS:
        if n == 1:
            rows = rng.choice(n_rows, 1)
        elif k == SEL_CAP and n > k:
            rows = np.concatenate([[lo, hi], rng.choice(below, k - 1, replace=False), rng.choice(above, n - k - 1, replace=False)])
        else:
            rest = np.setdiff1d(np.arange(n_rows), [lo, hi])
            rows = np.concatenate([[lo, hi], rng.choice(rest, n - 2, replace=False)])
        lists.append(np.sort(rows))
    return subset_blocks(base, lists, names=[f"{n}-{k}" for n, k in LIMITS])


BITONIC_N = (2049, 4096, 4097, 9000, 40000)


def bitonic_ks(n):
    """k > 2048: two fixed values (3000 > 2049 is cut to n) and the whole list."""
    return (2049, 3000, n)


def bitonic_case():
    """Lists for the global sort (k > 2048), padded to 4096, 4096, 8192, 16384 and 65536 keys."""
    base = distinct_rows()
    rng = np.random.default_rng(11)
    return subset_blocks(base, [np.sort(rng.choice(len(base.c), n, replace=False)) for n in BITONIC_N])


IDENTITY_K = (100, 2048, 2049)   # one-launch kernel, tournament, global sort


def identity_case():
    """9000 distinct finite distances on a dataset with identity ids, re-ranked as "all items" (no id list at all)."""
    case = distinct_rows(9000)
    case.ids = np.arange(len(case.c), dtype=np.uint32)
    return case


SUB_QUERIES, SUB_K, SUB_BIG = 1030, 1500, {5: 9000, 1027: 20000}
SUB_EMPTY = (0, 77, 1023, 1029)
SUB_PICKS = (5, 6, 77, 1022, 1023, 1024, 1027, 1028)


def sub_batch_case():
    """More than 1024 queries: ah_rerank_batch cuts the call after query 1023, and each part has its own key stride (the
    first is sized by query 5's 9000 candidates, the second by query 1027's 20 000)."""
    base = distinct_rows()
    rng = np.random.default_rng(3)
    n_rows = len(base.c)
    lists = []
    for q in range(SUB_QUERIES):
        n = SUB_BIG.get(q, 0 if q in SUB_EMPTY else int(rng.integers(3, 41)))
        lists.append(np.sort(rng.choice(n_rows, n, replace=False)))
    return subset_blocks(base, lists, names=[str(q) for q in range(SUB_QUERIES)])


# ---- case 2: the capacity edge of the selection --------------------------------------------------------------

CAP_K = 1000
SPREADS = ("consecutive", "span2048", "span2049", "wide")
SINGLE_SPREADS = SPREADS + ("wide-finite",)   # `wide` has NaN as its top word, which k_topk_small declines; this one does not


def _cycle(values, count):
    return np.resize(np.asarray(values, dtype=np.float32), count)


def capacity_case(k=CAP_K, spreads=SPREADS):
    """Per spread of the distance words, five lists at k (1000 by default: k - 1 keys below a tied word of multiplicity m):
    m = 1025 - k -> 1024 selected keys (the full sort width), m = 1026 - k -> 1025 (flagged), m = 1 -> exactly k;
    `bin0`: the k-th key is among k copies of the smallest word; `bin2047`: it is among 20 copies of the largest.
    Spread `wide-finite`: +0 ... f32::MAX (under ordinary ids), the widest span without a non-finite word."""
    assert 20 < k < SEL_CAP
    rng = np.random.default_rng(4)
    w0 = word_of(1.0)
    seqs, names = [], []
    for spread in spreads:
        if spread in ("wide", "wide-finite"):   # +0 ... NaN: a span of 2^31 words, 2^20 words (an eighth of a binade) per bin
            low = np.concatenate([[0.0], np.float32(2.0) ** np.arange(-100, -91, dtype=np.float32)]).astype(np.float32)
            tie = np.float32(1.0)
            high = np.float32(2.0) ** np.array([1, 50, 100], dtype=np.float32)
            top = np.float32(np.nan) if spread == "wide" else F32_MAX
        else:
            low, tie, high = f32(w0 + np.arange(10, dtype=np.uint32)), f32([w0 + 10])[0], f32(w0 + np.arange(11, 21, dtype=np.uint32))
            top = {"consecutive": f32([w0 + 20])[0], "span2048": f32([w0 + 2047])[0], "span2049": f32([w0 + 2048])[0]}[spread]
        for name, m in (("1024", SEL_CAP + 1 - k), ("1025", SEL_CAP + 2 - k), ("k", 1)):
            body = np.concatenate([_cycle(low, k - 1), _cycle([tie], m), _cycle(high, 2 * k - m)])
            rng.shuffle(body)
            # the largest word three times, inside the first 2k positions (a NaN there is never skipped)
            seqs.append(np.insert(body, [5, 50, 500], top))
            names.append(f"{spread}-{name}")
        body = np.concatenate([_cycle([low[0]], k), _cycle(high, 500), _cycle([top], 3)])
        rng.shuffle(body)
        seqs.append(body)
        names.append(f"{spread}-bin0")
        body = np.concatenate([_cycle(low, k - 10), _cycle([top], 20)])   # n = k + 10 <= 2k: nothing is skipped
        rng.shuffle(body)
        seqs.append(body)
        names.append(f"{spread}-bin2047")
    return Blocks(seqs, names)


# ---- case 3: ties ----------------------------------------------------------------------------------------

TIES_N, TIES_K = 9000, (1, 1024, 1025, 2048)
SINGLE_TIES_K = TIES_K + (2049,)   # ... and the global sort of the single-query path


def ties_case():
    rng = np.random.default_rng(5)
    halves = _cycle([2.0, 3.0], TIES_N)
    rng.shuffle(halves)
    return Blocks([_cycle([5.0], TIES_N), halves], ["all-equal", "two-values"])


# ---- cases 5 and 7: real kernel output ---------------------------------------------------------------------

BQ_K = (5, 1000, 2048)


def bq_case():
    """BinaryQuantizedEuclidean, 64 dims, 20 000 rows and 3 queries."""
    rng = np.random.default_rng(7)
    return rng.standard_normal((20000, 64)).astype(np.float32), rng.standard_normal((3, 64)).astype(np.float32)


def euclid_case():
    """Euclidean, 32 dims, 3000 rows and 6 queries."""
    rng = np.random.default_rng(8)
    return rng.standard_normal((3000, DIMS)).astype(np.float32), rng.standard_normal((6, DIMS)).astype(np.float32)


# ---- case 4: non-finite keys and the skip of src/reader.rs:611-621 ----------------------------------------------

NONFINITE_K = (8, 1100)   # selection (short lists, few selected keys) and tournament (k > 1024 flags every list)
SINGLE_NONFINITE_K = NONFINITE_K + (2100,)   # single query: the tournament twice (k_topk_small declines), then the global sort
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def _finite(rng, count, first_word=0x40000000):
    return f32(first_word + rng.permutation(count).astype(np.uint32))


def nonfinite_case(ks=NONFINITE_K):
    """For each k of `ks`, lists named `<k>-<what>`:
    skip-changes-answer     k-2 finite keys and k+2 NaNs in the first 2k positions, only +inf after them: the +inf are all
                            skipped and two NaNs are returned where a plain sort returns two +inf;
    late-admission          the same, then +inf, ONE finite key, +inf: the finite key ends the skipping, so the +inf after it
                            count (the regression input: skipping every such key from position 2k on returns a NaN instead);
    max-id-inside           n <= 2k, the list ends with (f32::MAX, id 0xFFFFFFFF), which is returned;
    max-id-skipped          the same item beyond position 2k with nothing finite before it there: skipped;
    max-id-admitted         (f32::MAX, an ordinary id) beyond 2k is below the threshold and ends the skipping, so the item
                            with id 0xFFFFFFFF after it counts;
    mixed                   finite keys everywhere, +inf / NaN / f32::MAX sprinkled: the rule changes nothing."""
    rng = np.random.default_rng(6)
    seqs, names, with_max = [], [], []

    def add(name, parts, max_id=False):
        if max_id:
            with_max.append(len(seqs))
        seqs.append(np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float32)) for p in parts]))
        names.append(name)

    for k in ks:
        def head(n_finite, extra=()):   # 2k positions: n_finite finite keys, `extra`, NaNs for the rest; shuffled
            h = np.concatenate([_finite(rng, n_finite), np.asarray(extra, dtype=np.float32)])
            h = np.concatenate([h, _cycle([NAN], 2 * k - len(h))])
            rng.shuffle(h)
            return h
        small = f32([0x3F000000])  # 0.5: below every key of _finite
        add(f"{k}-skip-changes-answer", [head(k - 2), _cycle([INF], 10)])
        add(f"{k}-late-admission", [head(k - 2), _cycle([INF], 3), small, _cycle([INF], 3), NAN])
        short = np.concatenate([_finite(rng, k - 3), [F32_MAX, INF, INF, NAN, NAN]]).astype(np.float32)
        rng.shuffle(short)
        add(f"{k}-max-id-inside", [short], max_id=True)            # n = k + 3 <= 2k
        add(f"{k}-max-id-skipped", [head(k - 3, [F32_MAX]), INF, INF], max_id=True)
        add(f"{k}-max-id-admitted", [head(k - 3, [F32_MAX]), INF, F32_MAX, INF], max_id=True)
        mixed = np.concatenate([_finite(rng, 3 * k), _cycle([INF, NAN, F32_MAX], 48)])
        rng.shuffle(mixed)
        add(f"{k}-mixed", [mixed], max_id=True)
    return Blocks(seqs, names, with_max_id=tuple(with_max))


# ---- single query: skippable keys across the blocks of the key-making kernels ------------------------------------------

FAR_RUN, FAR_TAIL = 9000, 5000
STRETCH = 1024      # positions one step of block_skip_end's walk covers: 256 threads, 4 positions each
KEY_BLOCKS = {"tournament": CHUNK, "bitonic": 256}     # positions per block of k_topk_round<true> / k_make_keys


def far_case(k):
    """One dataset per k with two lists, for the kernels of distance.hip in which every block finds skip_end for itself:
    `far`           2k positions (k - 6 finite keys, NaNs for the rest), then FAR_RUN +inf / NaN, all skipped (more than two
                    chunks of 4096 and many steps of the walk), then ONE finite key (skip_end, in a later block than the
                    first skipped keys), then FAR_TAIL keys that count: NaNs with two +inf right after skip_end, in its
                    block, and two +inf a chunk later.  The answer ends with those four +inf and one NaN of the head;
    `far-max-id`    the same rows and then the item (f32::MAX, id 0xFFFFFFFF), which counts as well."""
    rng = np.random.default_rng(12 + k)
    head = np.concatenate([_finite(rng, k - 6), _cycle([NAN], k + 6)])
    rng.shuffle(head)
    run = _cycle([INF, NAN, NAN], FAR_RUN)
    tail = _cycle([NAN], FAR_TAIL)
    tail[[3, 40, CHUNK + 5, CHUNK + 700]] = INF
    seq = np.concatenate([head, run, f32([0x3F000000]), tail])
    case = Blocks([seq], ["far"], with_max_id=(0,))
    return subset_blocks(case, [case.rows[0][:-1], case.rows[0]], ["far", "far-max-id"])


def skip_blocks(d, ids, k, block):
    """Restatement, for classification only, of what each block of `block` positions does in the key-making kernels: per
    block (wanted, what, steps).  wanted: it holds a skippable key at a position >= 2k, so it walks from 2k on; what: "all"
    (no key below the threshold before its end: its skippable keys are all skipped), "some" (skip_end lies inside it) or
    "none" (skip_end lies before it: nothing of it is skipped); steps: the steps of STRETCH positions its walk takes."""
    n, two_k = len(d), 2 * min(k, len(d))
    w = ordered_words(d)
    big = (w > MAX_WORD) | ((w == MAX_WORD) & (np.asarray(ids, dtype=np.uint64) == MAX_ID))
    below = np.flatnonzero(~big & (np.arange(n) >= two_k))
    skip_end = int(below[0]) if below.size else n + block
    out = []
    for base in range(0, n, block):
        end = min(n, base + block)
        wanted = bool(np.any(big[max(base, two_k):end]))
        what = "all" if skip_end >= end else "none" if skip_end <= base else "some"
        steps = -(-(min(skip_end + 1, end) - two_k) // STRETCH) if wanted else 0
        out.append((wanted, what, steps))
    return out


def agree(case, ks, picks=None):
    """The oracle's statement-by-statement median_based_top_k and the numpy `topk` give one answer on these lists."""
    from oracle import oracle as O
    od = O.Data(O.MANHATTAN, case.vectors, ids=case.ids)
    qv, qh = od.query_leaf(case.query)
    for i in (range(len(case)) if picks is None else picks):
        for k in ks:
            wi, wd = od.rerank(qv, qh, case.rows[i], k)
            ei, ed = case.expect(i, k)
            assert wi.tolist() == ei.tolist(), (case.names[i], k)
            assert canonical_bits(wd).tolist() == canonical_bits(ed).tolist(), (case.names[i], k)
