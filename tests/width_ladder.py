"""The width ladders of the hot kernels, restated in plain Python.

Nearly every hot kernel works in units of one 128-byte line (32 f32 dimensions, 2 words of a 1-bit row) and changes what it
does with the number of lines in a row: chunk sizes, ring refills, trips plus a remainder.  The functions below say, for a
width, which rung or branch of every such ladder it takes; tests/test_width_ladder_cpu.py asserts that the widths of
tests/test_gpu_widths.py take all of them, so a change to one of these constants that leaves a rung without a width fails on the
CPU and names the rung.  Every constant carries the place it restates (paths under arroy_amd/csrc)."""

LINE_DIMS = 32          # device_math.h:113  blocks = dims >> 5: a line of 32 f32 dimensions, the rest is the scalar tail
MAX_F32_DIMS = 1536     # the widest f32 row of the width tests (wider rows: a separate question)

# octet_wide_chunks: the margin of every descent (search.hip:145) and of k_route_items (forest.hip:1276)
WIDE_RUNGS = (48, 24, 12, 6, 3, 1)   # device_math.h:124 the chunk sizes; :165 each instantiation hands over to CH / 2
WIDE_START_LDS = 48                  # device_math.h:173 the query in LDS (descents with the query leaf in LDS) starts at 48 ...
WIDE_START_GLOBAL = 24               # device_math.h:173 ... both operands in global memory (routing, k_descend's global tier) at 24
WIDE_GROUP = 8                       # device_math.h:146 LDS query: multiply-adds in groups of G = 8 when 8 divides CH, else one of CH

RING_DEPTH = 6          # search.hip:2299-2300 leaf_tile_ring<METRIC, QO, 6>: steps in the LDS ring (:2217 prologue, :2224 refill)
FLY = 8                 # device_math.h:182 octet_reduce_stream: line loads in flight, then a remainder loop (:200)
KF_ONE_VISIT = 24       # search.hip:2520, :2607 leaf_tile16<2, 1, 1, 24>: steps requested together, units of one visit
KF_TWO_VISITS = 12      # search.hip:2613 leaf_tile16<2, 2, 1, 12>: units of two visits
HALF_STEP = 64          # search.hip:2413 steps = hpitch >> 6: a step of leaf_tile16 is one line of 64 halves
HPITCH_ALIGN = 64       # forest.hip:2073 hpitch = round_up(dims, 64)
PITCH8_ALIGN = 128      # forest.hip:2133 pitch8 = round_up(dims, 128)
PAIR_LINES = 2          # batch.hip:402 k_pairs_distances_runs: lines in pairs, :416 the odd one

BQ_WORD_BITS = 64       # binary_quantized.rs:67-69 words = ceil(dims / 64)
BQ_PITCH_ALIGN = 2      # ah_dataset_create: pitch = round_up(words, 2): rows of whole 16-byte chunks, an odd word count gets a zero word
BQ_UNROLL = 8           # distance.hip:291 kBqUnroll: chunk loads in flight per trip
BQ_MAX_CHUNKS = 32      # distance.hip:290 kBqMaxChunks (:433 wider rows take k_distances_bq_wide)
BQ_TILE_ROWS = 64       # distance.hip:321 a wave's tile: step_r = 64 / C rows, step_p = 64 % C parts per load

LDS_DEFAULT_LIMIT = 48 * 1024   # forest.hip:2952, split.hip:139 more dynamic LDS than this needs the opt-in
SPLIT_BUFFERS = 3               # forest.hip:2941, split.hip:136 three centroid-sized f32 buffers of the two-means

F32_WIDTHS = (160, 192, 232, 288, 384, 416, 520, 736, 800, 1000, 1024, 1504, 1536)
F32_WIDTHS_ALL_METRICS = (192, 384, 736, 1024, 1504)   # DotProduct and Manhattan as well as Euclidean and Cosine
BQ_WIDTHS = (192, 400, 640, 1100, 1536, 3072, 4032, 4160)
BQ_WIDTHS_ALL_METRICS = (192, 1536, 4160)              # all three 1-bit metrics (elsewhere BinaryQuantizedCosine and one more)


def round_up(x, to):
    return (x + to - 1) // to * to


def lines(dims):
    return dims // LINE_DIMS


def wide_chunks(n_lines, lds):
    """The chunks octet_reduce_wide takes for a row of n_lines, in order."""
    out, k = [], 0
    ch = WIDE_START_LDS if lds else WIDE_START_GLOBAL
    while True:
        while k + ch <= n_lines:
            out.append(ch)
            k += ch
        if ch == 1:
            return out
        ch //= 2


def wide_groups(ch):
    """(G, NG) of a chunk whose query is in LDS."""
    g = WIDE_GROUP if ch % WIDE_GROUP == 0 else ch
    return g, ch // g


def wide_hand_overs(n_lines, lds):
    """Pairs (a, b) of different rungs taken one after the other."""
    c = wide_chunks(n_lines, lds)
    return {(a, b) for a, b in zip(c, c[1:]) if a != b}


def ring_events(n_lines):
    """What the ring of leaf_tile_ring goes through for a row of n_lines steps."""
    ev = set()
    if n_lines < RING_DEPTH - 1:
        ev.add("prologue cut short")
    if n_lines == RING_DEPTH - 1:
        ev.add("prologue exact, never refilled")
    if n_lines == RING_DEPTH:
        ev.add("one refill, no slot reused")
    if n_lines == RING_DEPTH + 1:
        ev.add("first slot reused once")
    if n_lines >= 2 * RING_DEPTH + 1:
        ev.add("a slot reused twice")
    return ev


def trips(n, per):
    """'full' (whole trips only), 'rest' (a remainder only), 'both' or 'none' of a loop of `per` with a remainder loop."""
    full, rest = n // per, n % per
    return "none" if n == 0 else "full" if rest == 0 else "rest" if full == 0 else "both"


def hpitch(dims):
    return round_up(dims, HPITCH_ALIGN)


def pitch8(dims):
    return round_up(dims, PITCH8_ALIGN)


def tile16_steps(dims):
    return hpitch(dims) // HALF_STEP


def bq_words(dims):
    return (dims + BQ_WORD_BITS - 1) // BQ_WORD_BITS


def bq_pitch(dims):
    return round_up(bq_words(dims), BQ_PITCH_ALIGN)


def bq_chunks(dims):
    """C: 16-byte chunks per row."""
    return bq_pitch(dims) // 2


def bq_cooperative(dims):
    return bq_chunks(dims) <= BQ_MAX_CHUNKS


def split_lds_bytes(dims, one_bit):
    """Dynamic LDS of the two-means: three buffers of f32_space_pitch floats (split_device.h:29-34)."""
    space = bq_words(dims) * BQ_WORD_BITS if one_bit else dims
    return SPLIT_BUFFERS * round_up(space, LINE_DIMS) * 4


def split_needs_opt_in(dims, one_bit):
    return split_lds_bytes(dims, one_bit) > LDS_DEFAULT_LIMIT
