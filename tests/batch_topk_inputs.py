"""Designed inputs for the batched top-k of ah_rerank_batch (arroy_amd/csrc/batch.hip), shared by test_batch_topk_cpu.py
(which proves on the CPU that every input has the property it is named for) and test_gpu_batch_topk.py (which runs them).

The device that makes the inputs exact: a Manhattan dataset of 32 dims whose rows are (c, 0, ..., 0) and an all-zero query,
so that the distance of a row is |c| bit for bit and a test chooses every distance word.  Candidate lists are ascending in
id, hence in row: a list's distance sequence is laid out as a block of consecutive rows (`Blocks`).

Two restatements live here, written from the comments and constants of batch.hip and used ONLY to classify inputs ("this
query must be left to the tournament", "this list takes 4 rounds"), never as an expected answer:
  `tour_rounds`   chunks of 4096 keys, each block keeps min(k, 2048), the last block keeps k;
  `selection`     2048 bins over the span of the distance words (direct when the span is <= 2048, else
                  scale = floor(2048 * 2^32 / span)), the bin of the k-th key, and the count of keys up to that bin.
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


def selection(d, ids, k):
    """What k_batch_topk_select computes before it sorts: span, direct / scaled, the k-th key's bin, n_sel, flagged."""
    n = len(d)
    kk = min(k, n)
    w = ordered_words(d)
    w[skipped(d, ids, k)] = 0xFFFFFFFF      # a skipped key is the sentinel, whose word takes part in the span
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


def subset_blocks(blocks, row_lists, names=None):
    """Lists that are ascending subsets of one dataset's rows instead of its blocks."""
    b = Blocks.__new__(Blocks)
    b.c, b.ids, b.vectors, b.query = blocks.c, blocks.ids, blocks.vectors, blocks.query
    b.rows = [np.ascontiguousarray(r, dtype=np.uint32) for r in row_lists]
    b.names = list(names) if names is not None else [str(len(r)) for r in b.rows]
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


def _cycle(values, count):
    return np.resize(np.asarray(values, dtype=np.float32), count)


def capacity_case():
    """Per spread of the distance words, five lists at k = 1000 (999 keys below a tied word of multiplicity m):
    m = 25 -> 1024 selected keys (the full sort width), m = 26 -> 1025 (flagged), m = 1 -> exactly k;
    `bin0`: the k-th key is among 1000 copies of the smallest word; `bin2047`: it is among 20 copies of the largest."""
    rng = np.random.default_rng(4)
    w0 = word_of(1.0)
    seqs, names = [], []
    for spread in SPREADS:
        if spread == "wide":   # +0 ... NaN: a span of 2^31 words, 2^20 words (an eighth of a binade) per bin
            low = np.concatenate([[0.0], np.float32(2.0) ** np.arange(-100, -91, dtype=np.float32)]).astype(np.float32)
            tie = np.float32(1.0)
            high = np.float32(2.0) ** np.array([1, 50, 100], dtype=np.float32)
            top = np.float32(np.nan)
        else:
            low, tie, high = f32(w0 + np.arange(10, dtype=np.uint32)), f32([w0 + 10])[0], f32(w0 + np.arange(11, 21, dtype=np.uint32))
            top = {"consecutive": f32([w0 + 20])[0], "span2048": f32([w0 + 2047])[0], "span2049": f32([w0 + 2048])[0]}[spread]
        for name, m in (("1024", 25), ("1025", 26), ("k", 1)):
            body = np.concatenate([_cycle(low, CAP_K - 1), _cycle([tie], m), _cycle(high, 2000 - m)])
            rng.shuffle(body)
            # the largest word three times, inside the first 2k positions (a NaN there is never skipped)
            seqs.append(np.insert(body, [5, 50, 500], top))
            names.append(f"{spread}-{name}")
        body = np.concatenate([_cycle([low[0]], CAP_K), _cycle(high, 500), _cycle([top], 3)])
        rng.shuffle(body)
        seqs.append(body)
        names.append(f"{spread}-bin0")
        body = np.concatenate([_cycle(low, CAP_K - 10), _cycle([top], 20)])   # n = 1010 <= 2k: nothing is skipped
        rng.shuffle(body)
        seqs.append(body)
        names.append(f"{spread}-bin2047")
    return Blocks(seqs, names)


# ---- case 3: ties ----------------------------------------------------------------------------------------

TIES_N, TIES_K = 9000, (1, 1024, 1025, 2048)


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
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def _finite(rng, count, first_word=0x40000000):
    return f32(first_word + rng.permutation(count).astype(np.uint32))


def nonfinite_case():
    """For each k of NONFINITE_K, lists named `<k>-<what>`:
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

    for k in NONFINITE_K:
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
