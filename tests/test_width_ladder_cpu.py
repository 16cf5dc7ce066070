"""The widths of tests/test_gpu_widths.py against the ladders of tests/width_ladder.py: together they take every rung, every
hand-over and every branch the kernels have for rows of up to 1536 f32 dimensions and for 1-bit rows.  A ladder constant that
changes so that a rung is left without a width fails here, without a GPU, and the message names the rung."""
import width_ladder as W


def need(wanted, seen, what):
    missing = [w for w in wanted if w not in seen]
    assert not missing, f"{what}: no width takes {missing} (taken: {sorted(seen, key=str)})"


def test_width_lists_are_what_the_gpu_module_runs():
    assert list(W.F32_WIDTHS) == sorted(set(W.F32_WIDTHS)) and max(W.F32_WIDTHS) == W.MAX_F32_DIMS
    assert set(W.F32_WIDTHS_ALL_METRICS) <= set(W.F32_WIDTHS) and set(W.BQ_WIDTHS_ALL_METRICS) <= set(W.BQ_WIDTHS)
    # lines + scalar tail of the f32 widths, words and chunks of the 1-bit widths
    assert [(W.lines(d), d % W.LINE_DIMS) for d in W.F32_WIDTHS] == [
        (5, 0), (6, 0), (7, 8), (9, 0), (12, 0), (13, 0), (16, 8), (23, 0), (25, 0), (31, 8), (32, 0), (47, 0), (48, 0)]
    assert [(W.bq_words(d), W.bq_chunks(d)) for d in W.BQ_WIDTHS] == [
        (3, 2), (7, 4), (10, 5), (18, 9), (24, 12), (48, 24), (63, 32), (65, 33)]


def test_wide_chunk_ladder_every_rung_and_hand_over():
    assert W.WIDE_RUNGS[0] == W.WIDE_START_LDS and W.WIDE_START_GLOBAL in W.WIDE_RUNGS
    assert all(b == a // 2 for a, b in zip(W.WIDE_RUNGS, W.WIDE_RUNGS[1:])), "each instantiation hands over to CH / 2"
    for lds, widths in ((True, W.F32_WIDTHS), (False, W.F32_WIDTHS), (True, W.F32_WIDTHS_ALL_METRICS), (False, W.F32_WIDTHS_ALL_METRICS)):
        start = W.WIDE_START_LDS if lds else W.WIDE_START_GLOBAL
        # (the margins are dot products whatever the metric; the top rung, 48 lines, is taken at 1536, where Euclidean and Cosine run)
        rungs = [r for r in W.WIDE_RUNGS if r <= (start if widths is W.F32_WIDTHS else W.WIDE_START_GLOBAL)]
        taken, overs, repeated = set(), set(), set()
        for d in widths:
            c = W.wide_chunks(W.lines(d), lds)
            assert sum(c) == W.lines(d) and c == sorted(c, reverse=True), (d, c)
            taken |= set(c)
            overs |= W.wide_hand_overs(W.lines(d), lds)
            repeated |= {a for a, b in zip(c, c[1:]) if a == b}
        what = f"octet_wide_chunks, query in {'LDS' if lds else 'global memory'}, widths {widths}"
        need(rungs, taken, what + ", rung")
        # every hand-over between neighbouring rungs that a row of at most 48 lines can take: the top rung of the LDS ladder
        # is left only by rows of 72 lines or more (2304 dimensions)
        reachable = [(a, b) for a, b in zip(rungs, rungs[1:]) if a + b <= W.lines(W.MAX_F32_DIMS)]
        need(reachable, overs, what + ", hand-over to the next rung")
        assert any(W.WIDE_RUNGS.index(b) - W.WIDE_RUNGS.index(a) > 1 for a, b in overs), what + ": no width skips a rung"
        assert repeated, what + ": no width takes a rung twice"
    # the LDS query's groups: one group (G = CH), two groups (double buffer used once) and more
    groups = {W.wide_groups(c) for d in W.F32_WIDTHS for c in W.wide_chunks(W.lines(d), True)}
    need([(8, 6), (8, 3), (12, 1), (6, 1), (3, 1), (1, 1)], groups, "octet_wide_chunks (G, NG)")
    # rungs a search took before these widths (dims <= 100, 256, 768, 1536): 12 and the mixed decompositions were not among them
    assert W.wide_chunks(12, True) == [12] and W.wide_chunks(16, True) == [12, 3, 1] and W.wide_chunks(47, True) == [24, 12, 6, 3, 1, 1]


def test_ring_refills():
    for widths in (W.F32_WIDTHS,):  # Euclidean and Cosine run at every width
        ev = set().union(*(W.ring_events(W.lines(d)) for d in widths))
        need(["prologue exact, never refilled", "one refill, no slot reused", "first slot reused once", "a slot reused twice"], ev,
             "leaf_tile_ring")
    assert {W.lines(d) for d in W.F32_WIDTHS} >= {W.RING_DEPTH - 1, W.RING_DEPTH, W.RING_DEPTH + 1}
    assert any(W.lines(d) >= 13 for d in W.F32_WIDTHS)
    # DotProduct re-ranks through the ring with the screen off: refilled rings there too
    assert any("a slot reused twice" in W.ring_events(W.lines(d)) for d in W.F32_WIDTHS_ALL_METRICS)
    assert any("one refill, no slot reused" in W.ring_events(W.lines(d)) for d in W.F32_WIDTHS_ALL_METRICS)


def test_tile16_trips_and_padding():
    for kf in (W.KF_ONE_VISIT, W.KF_TWO_VISITS):
        seen = {W.trips(W.tile16_steps(d), kf) for d in W.F32_WIDTHS}
        # (whole trips AND a remainder of KF = 24 need more than 24 steps: rows beyond 1536 dimensions)
        wanted = ["full", "rest"] + (["both"] if W.tile16_steps(W.MAX_F32_DIMS) > kf else [])
        need(wanted, seen, f"leaf_tile16, KF = {kf}")
    assert W.trips(W.tile16_steps(W.MAX_F32_DIMS), W.KF_TWO_VISITS) != "rest"
    need(["full", "rest", "both"], {W.trips(W.tile16_steps(d), kf) for d in W.F32_WIDTHS for kf in (W.KF_ONE_VISIT, W.KF_TWO_VISITS)},
         "leaf_tile16, any KF")
    assert 16 in {W.tile16_steps(d) for d in W.F32_WIDTHS}, "a row of 16 steps: 12 + 4 left over"
    # binary16 rows whose last half line is padding, and rows that end inside a line
    pads = {W.hpitch(d) - d for d in W.F32_WIDTHS}
    need([0, 32], pads, "hpitch - dims")
    assert any(0 < p < 32 for p in pads) and sum(1 for d in W.F32_WIDTHS if W.hpitch(d) - d == 32) >= 3
    # the int8 copy: pitch8 a multiple of 128 beyond dims by 0, by whole lines of 32 and by a ragged rest
    pads8 = {W.pitch8(d) - d for d in W.F32_WIDTHS}
    need([0, 32, 64, 96], pads8, "pitch8 - dims")
    assert any(p % 32 for p in pads8)
    for d in W.F32_WIDTHS_ALL_METRICS:  # DotProduct is screened as well
        assert W.hpitch(d) >= d and W.pitch8(d) >= d
    assert {W.hpitch(d) - d for d in W.F32_WIDTHS_ALL_METRICS} >= {0, 32}


def test_stream_and_pair_loops():
    for widths in (W.F32_WIDTHS, W.F32_WIDTHS_ALL_METRICS):
        need(["full", "rest", "both"], {W.trips(W.lines(d), W.FLY) for d in widths}, f"octet_reduce_stream (FLY = {W.FLY}), widths {widths}")
        need(["full", "both"], {W.trips(W.lines(d), W.PAIR_LINES) for d in widths}, f"k_pairs_distances_runs, widths {widths}")
    assert any(d % W.LINE_DIMS for d in W.F32_WIDTHS), "no width with a scalar tail"


def test_one_bit_ladders():
    for widths in (W.BQ_WIDTHS, W.BQ_WIDTHS_ALL_METRICS):
        words = [W.bq_words(d) for d in widths]
        assert any(w % 2 for w in words) and any(w % 2 == 0 for w in words), f"odd and even word counts, widths {widths}"
        assert any(W.bq_cooperative(d) for d in widths) and any(not W.bq_cooperative(d) for d in widths), widths
        opt = {W.split_needs_opt_in(d, True) for d in widths}
        need([True, False], opt, f"LDS opt-in of the two-means, widths {widths}")
    cs = [W.bq_chunks(d) for d in W.BQ_WIDTHS]
    assert any(W.BQ_TILE_ROWS % c for c in cs if c <= W.BQ_MAX_CHUNKS), "no C with 64 % C != 0: the row / part carry never runs"
    assert any(W.BQ_TILE_ROWS % c == 0 for c in cs)
    assert any(W.BQ_UNROLL < c <= 2 * W.BQ_UNROLL for c in cs), "C in (8, 16]"
    assert any(2 * W.BQ_UNROLL < c <= 3 * W.BQ_UNROLL for c in cs), "C in (16, 24]"
    assert W.BQ_MAX_CHUNKS in cs and W.BQ_MAX_CHUNKS + 1 in cs, "the last cooperative width and the first wide one"
    need(["full", "rest", "both"], {W.trips(c, W.BQ_UNROLL) for c in cs if c <= W.BQ_MAX_CHUNKS}, "k_distances_bq trips of kBqUnroll")
    assert any(d % W.BQ_WORD_BITS for d in W.BQ_WIDTHS), "no width with tail bits in its last word"
    # the opt-in sits just past the limit at the first wide width, while the stored row stays small
    assert W.split_lds_bytes(4160, True) == 49920 > W.LDS_DEFAULT_LIMIT and W.bq_pitch(4160) * 8 == 528
    # ... and no f32 width of the module reaches it (an f32 row of 4160 dimensions is out of its scope)
    assert not any(W.split_needs_opt_in(d, False) for d in W.F32_WIDTHS)
