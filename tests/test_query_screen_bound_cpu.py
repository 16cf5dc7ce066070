"""The certified top-k screens of the query side, restated in numpy and checked against the ORACLE's f32 distances (no GPU).

ah_search_batch and ah_rerank_batch (Cosine / DotProduct) score every candidate on a coarse copy of the rows first — the
binary16 copy, or the int8 copy before it — and derive an interval L <= d_ref <= U from a proven bound E >= |s - r| on the
distance of the screen value s to the reference's f32 dot product r (arroy_amd/csrc/search.hip:
k_queries_h16 / query_h16, query_i8, k_pairs_screen16 / 8, screened_error, screened_bounds, the int8 E in
search_select_screened_body; forest.hip: k_shadow_rows, k_stats_max, k_col_maxabs, k_dim_scales, k_shadow_rows8).  Only
the candidates whose L reaches the k-th smallest U are evaluated in f32, so an E that is too small for some input drops a
true top-k member without any error.

This test rebuilds both copies, both bounds and the interval in float32 arithmetic as the kernels do, takes d_ref from
the oracle (the reference's own summation order) and asserts L <= d_ref <= U for every (query, row) pair whose screen
value is finite — for the exact screen value and for f32 sums in the kernels' lane order, in sequence and reversed (E
claims to cover any order).  A screen value that is not finite must be recognised as such (the selection then sends the
submission to the exact path).  The largest |s - r| / E per case is printed: which inputs actually press on the bound."""
import numpy as np
import pytest

from oracle import oracle as O

F = np.float32
TINY = F(2.0 ** -40)           # kTinyBits (screen_device.h)
HALF_MIN = F(6.103515625e-05)  # to_shadow_half: binary16 subnormals become 0


def up(pitch):
    return F(1.0) + F(pitch + 64) * F(1.2e-7)


def f32norm(v):
    return np.sqrt((v.astype(F) * v.astype(F)).sum(axis=-1, dtype=F)).astype(F)


def row_pitch(dims):
    return (dims + 31) // 32 * 32


def gammas(dims):
    hpitch = (dims + 63) // 64 * 64
    return F(4.0 * (2.0 * (hpitch // 16) + 8.0) * 5.9604645e-8), F(4.0 * ((dims // 32) + 6.0 + 62.0) * 5.9604645e-8)


def shadow(v):
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    h[np.abs(h.astype(F)) < HALF_MIN] = 0
    return h


def cosine_from_dot(pq, pn, qn):
    """device_math.h: cosine.rs:43-59 in f32, elementwise."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pnqn = (pn * qn).astype(F)
        c = (pq / pnqn).astype(F)
        c = np.where(c < F(-1.0), F(-1.0), c)
        c = np.where(c > F(1.0), F(1.0), c)
        d = ((F(1.0) - c) / F(2.0)).astype(F)
    return np.where(pnqn > F(1.1920929e-7), d, F(0.0)).astype(F)


def interval(metric, s, e_query, qn, xn):
    """screened_bounds<METRIC>."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = (e_query + F(2.4e-7) * np.abs(s) + F(1e-30)).astype(F)
        r_lo, r_hi = (s - e).astype(F), (s + e).astype(F)
    if metric == O.DOT_PRODUCT:
        return -r_hi, -r_lo, e
    return cosine_from_dot(r_hi, xn, qn), cosine_from_dot(r_lo, xn, qn), e


# ---- the binary16 stage --------------------------------------------------------------------------------------------

def rows16(X):
    """k_shadow_rows + k_stats_max: the copy and the dataset-wide maxima of {|x~|, |x - x~|, |x|} (inf for tiny rows)."""
    dims = X.shape[1]
    Xh = shadow(X)
    xf = Xh.astype(F)
    u = up(row_pitch(dims))
    with np.errstate(over="ignore", invalid="ignore"):
        st = np.stack([f32norm(xf) * u, f32norm((X - xf).astype(F)) * u, f32norm(X) * u], axis=1).astype(F)
    xm = np.abs(X).max(axis=1)
    tiny = (xm != 0) & (xm < TINY)
    st[tiny] = np.inf
    return Xh, st.max(axis=0).astype(F)  # (k_stats_max takes the maximum of the bit patterns: a NaN ends up on top)


def query16(q, dims):
    """query_h16: the binary16 copy and {|q~|, |q - q~|, |q|} rounded up (inf for a tiny query)."""
    hpitch = (dims + 63) // 64 * 64
    qh = shadow(q)
    y = qh.astype(F)
    u = up(hpitch)
    with np.errstate(over="ignore", invalid="ignore"):
        st = np.array([f32norm(y) * u, f32norm((q - y).astype(F)) * u, f32norm(q) * u], dtype=F)
    m = np.abs(q).max()
    if m != 0 and m < TINY:
        st[:] = np.inf
    return qh, st


def screened_error(rs, qs, dims):
    g_s, g_r = gammas(dims)
    with np.errstate(invalid="ignore", over="ignore"):
        return F((g_s * (qs[0] * rs[0]) + qs[1] * rs[0] + qs[2] * rs[1] + g_r * (qs[2] * rs[2])) * F(1.002))


def lane_sums(P, width):
    """f32 sums of per-element products in the kernels' shape: lane j of an octet owns the pieces j, j + 8, ... of `width`
    elements each, accumulates them in sequence, and octet_sum adds the 8 lanes as a butterfly."""
    n, m = P.shape
    pieces = m // width
    lanes = np.zeros((n, 8), dtype=F)
    for p in range(pieces):
        lanes[:, p % 8] = (lanes[:, p % 8] + P[:, p * width:(p + 1) * width].sum(axis=1, dtype=np.float64).astype(F)).astype(F)
    a = (lanes[:, 0::2] + lanes[:, 1::2]).astype(F)
    b = (a[:, 0::2] + a[:, 1::2]).astype(F)
    return (b[:, 0] + b[:, 1]).astype(F)


def screen16_values(Xh, qh):
    """The screen value in several f32 orders, and exactly (f64 of the exact binary16 products)."""
    xf, qf = Xh.astype(np.float64), qh.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        P = (xf * qf).astype(F)  # exact: 11-bit x 11-bit significands
        return {
            "exact": (xf @ qf).astype(F),
            "lanes": lane_sums(P, 8),
            "sequential": np.cumsum(P, axis=1, dtype=F)[:, -1],
            "reversed": np.cumsum(P[:, ::-1], axis=1, dtype=F)[:, -1],
        }


# ---- the int8 stage -------------------------------------------------------------------------------------------------

def dim_scales(X, pitch8):
    """k_col_maxabs + k_dim_scales: per column the power of two >= its largest |x| (1 beyond 2^+-63, empty, non-finite)."""
    d = np.ones(pitch8, dtype=F)
    bits = (np.abs(X).astype(F)).view(np.uint32).max(axis=0)
    e = (bits >> 23).astype(np.int64) + ((bits & 0x7FFFFF) != 0)
    ok = (bits != 0) & (bits < 0x7F800000) & (e >= 64) & (e <= 190)
    d[: X.shape[1]][ok] = np.ldexp(F(1.0), (e[ok] - 127).astype(np.int32)).astype(F)
    return d


def rows8(X):
    """k_shadow_rows8: int8 digits per row, s_r (0: all zero, inf: not usable), and the maxima of {|q|, |y/s - q|, |x|/s}."""
    n, dims = X.shape
    pitch8 = (dims + 127) // 128 * 128
    pitch = row_pitch(dims)
    d = dim_scales(X, pitch8)
    Y = (X * (F(1.0) / d[:dims])).astype(F)  # exact
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.abs(Y).max(axis=1).astype(F)
        xm = np.abs(X).max(axis=1).astype(F)
    ok = (m >= TINY) & (xm >= TINY) & np.isfinite(m) & np.isfinite(xm)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = np.where(ok, m / F(127.0), F(0.0)).astype(F)
        inv = np.where(ok, F(127.0) / m, F(0.0)).astype(F)
        q = np.where(ok[:, None], np.clip(np.rint((Y * inv[:, None]).astype(F)), -127, 127), 0).astype(np.int32)
        z = (q.astype(F) * scale[:, None]).astype(F)
        u = up(pitch) * F(1.000001)
        sa = np.sqrt((q.astype(np.int64) ** 2).sum(axis=1).astype(F)).astype(F) * u
        sb = f32norm(np.where(ok[:, None], Y - z, F(0.0)).astype(F)) * u
        sc = f32norm(np.where(ok[:, None], X, F(0.0))) * u
        mb = ((sb + F(127.0) * scale * F(6.0e-8) * np.sqrt(F(pitch))) / scale * F(1.000001)).astype(F)
        mc = (sc / scale * F(1.000001)).astype(F)
    s_r = np.where(ok, scale, np.where(xm == 0, F(0.0), F(np.inf))).astype(F)
    q = np.pad(q, ((0, 0), (0, pitch8 - dims)))  # the zero tail of the int8 rows
    mx = np.array([sa[ok].max(), mb[ok].max(), mc[ok].max()], dtype=F) if ok.any() else np.zeros(3, F)
    return q, s_r, d, mx, ok


def query8(v, d, mx, dims):
    """query_i8: two int8 digits of q' = q o d, s_q, and A_q (0 for a zero query, inf for a tiny / non-finite one)."""
    pitch8 = d.size
    x0 = np.zeros(pitch8, F)
    x0[:dims] = v
    x = (x0 * d).astype(F)
    mbits = np.abs(x).view(np.uint32).max()
    m = np.abs(x).max()
    ok = mbits >= TINY.view(np.uint32) and mbits < 0x7F800000
    scale = F(m / F(127.0)) if ok else F(0.0)
    inv = F(F(127.0) / m) if ok else F(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x * inv).astype(F)
        qh = np.clip(np.rint(t), -127, 127).astype(np.int32) if ok else np.zeros(pitch8, np.int32)
        ql = np.clip(np.rint(((t - qh.astype(F)) * F(256.0)).astype(F)), -127, 127).astype(np.int32) if ok else np.zeros(pitch8, np.int32)
        y = ((qh.astype(F) + ql.astype(F) * F(0.00390625)) * scale).astype(F)
        u = up(pitch8)
        an, cn, cn0 = f32norm(y) * u, f32norm(x) * u, f32norm(x0) * u
        bn = f32norm((x - y).astype(F)) * u + F(128.0) * scale * F(6.0e-8) * np.sqrt(F(pitch8)) if ok else \
            (F(0.0) if mbits == 0 else F(np.inf))
        _, g_r = gammas(dims)
        a = F((bn * mx[0] + cn * mx[1] + F(2.0e-6) * (an * mx[0]) + g_r * (cn0 * mx[2])) * F(1.000001) * F(1.002))
    return qh, ql, scale, a


def screen8_values(q8, s_r, qh, ql, s_q):
    H = (q8.astype(np.int64) * qh[None, :]).astype(np.float64)
    L = (q8.astype(np.int64) * ql[None, :]).astype(np.float64)
    pitch8 = qh.size
    with np.errstate(invalid="ignore", over="ignore"):
        exact = ((H.sum(axis=1) + L.sum(axis=1) / 256.0) * float(s_q) * s_r.astype(np.float64)).astype(F)
        # k_pairs_screen8: lane j owns the 16-byte pieces j, j + 8, ...: exact integer sums per lane, then f32
        lane_of = (np.arange(pitch8) // 16) % 8
        Hl = np.stack([H[:, lane_of == j].sum(axis=1) for j in range(8)], axis=1)
        Ll = np.stack([L[:, lane_of == j].sum(axis=1) for j in range(8)], axis=1)
        lanes = (Hl.astype(F) + Ll.astype(F) * F(0.00390625)).astype(F)
        a = (lanes[:, 0::2] + lanes[:, 1::2]).astype(F)
        b = (a[:, 0::2] + a[:, 1::2]).astype(F)
        v = (b[:, 0] + b[:, 1]).astype(F)
        lane = ((v * s_q).astype(F) * s_r).astype(F)
        P = (H + L / 256.0).astype(F)
        seq = ((np.cumsum(P, axis=1, dtype=F)[:, -1] * s_q).astype(F) * s_r).astype(F)
    return {"exact": exact, "lanes": lane, "sequential": seq}


# ---- the cases ------------------------------------------------------------------------------------------------------

def case_data(name, dims, rng):
    """(rows, queries) of one distribution."""
    n, nq = 500, 5
    G = lambda *s: rng.standard_normal(s).astype(F)  # noqa: E731
    if name == "uniform":
        X, Q = rng.uniform(-1, 1, (n, dims)).astype(F), rng.uniform(-1, 1, (nq, dims)).astype(F)
    elif name == "gaussian":
        X, Q = G(n, dims), G(nq, dims)
    elif name == "clustered":
        X = O.synth(5, 4, n, dims)
        Q = np.stack([X[3], X[:50].mean(axis=0), X[100] + G(dims) * F(0.01), G(dims), X[:20].mean(axis=0)]).astype(F)
    elif name == "low-rank":
        X = O.synth(6, 5, n, dims)
        Q = np.concatenate([X[:2], G(3, dims)]).astype(F)
    elif name == "near-duplicates":
        base = G(dims)
        X = np.repeat(base[None], n, axis=0)
        X[: n // 2] = X[: n // 2] * (F(1.0) + G(n // 2, dims) * F(3e-7))   # a few ulps
        X[n // 2:] = X[n // 2:] + G(n - n // 2, dims) * F(1e-3)            # below the int8 step
        X = X.astype(F)
        Q = np.stack([base, X[7], X.mean(axis=0), G(dims), base * F(-1.0)]).astype(F)
    elif name == "column scales 2^+-20":
        X, Q = G(n, dims), G(nq, dims)
        s = np.ones(dims, F)
        s[::3], s[1::3] = F(2.0 ** 20), F(2.0 ** -20)
        X, Q = (X * s).astype(F), (Q * s).astype(F)
    elif name == "norms 1e-3..1e3":
        X = (G(n, dims) * np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 1)))).astype(F)
        Q = np.concatenate([X[:2], G(3, dims)]).astype(F)
    elif name == "zero rows and query":
        X = G(n, dims)
        X[::7] = 0.0
        Q = np.concatenate([np.zeros((1, dims), F), G(4, dims)]).astype(F)
    elif name == "binary16 subnormal range":
        X = (G(n, dims) * F(3e-5)).astype(F)
        X[::2] *= F(100.0)
        Q = np.concatenate([G(3, dims) * F(2e-5), X[1:3]]).astype(F)
    elif name == "tiny rows":
        X = G(n, dims)
        X[0] *= F(2.0 ** -44)   # below kTinyBits
        X[1] *= F(2.0 ** -38)   # just above
        Q = G(nq, dims)
    elif name == "beyond 65504":
        X = G(n, dims)
        X[3, 0] = F(1e5)
        X[4, 1] = F(np.inf)
        Q = np.concatenate([G(4, dims), (G(1, dims) * F(1e5))]).astype(F)
    else:
        raise AssertionError(name)
    return X.astype(F), Q.astype(F)


CASES = ["uniform", "gaussian", "clustered", "low-rank", "near-duplicates", "column scales 2^+-20", "norms 1e-3..1e3",
         "zero rows and query", "binary16 subnormal range", "tiny rows", "beyond 65504"]
WORST = {}


@pytest.mark.parametrize("metric", [O.COSINE, O.DOT_PRODUCT], ids=["cosine", "dot"])
@pytest.mark.parametrize("dims", [32, 96, 768, 1536])
@pytest.mark.parametrize("name", CASES)
def test_query_screen_interval_holds(name, dims, metric):
    rng = np.random.default_rng(abs(hash((name, dims))) % (2 ** 32))
    X, Q = case_data(name, dims, rng)
    data = O.Data(metric, X)
    if metric == O.DOT_PRODUCT:
        data.preprocess_dot()
    dot = O.Data(O.DOT_PRODUCT, X)  # the reference dot product r (same summation as the metric's: spaces/simple.rs)
    xn = data.headers[:, 0].astype(F)
    Xh, rmax = rows16(X)
    q8, s_r, dsc, mx8, _ok8 = rows8(X)
    int8_kept = bool(np.isfinite(mx8).all() and mx8[0] > 0)  # ensure_screen8: the copy exists only then
    worst = {"binary16": 0.0, "int8": 0.0}
    checked = 0
    for q in Q:
        qv, qh_hdr = data.query_leaf(q)
        d_ref = data.distances(qv, qh_hdr)
        r_ref = -dot.distances(*dot.query_leaf(q))
        qn = F(qh_hdr[0])
        stages = []
        qh16, qs16 = query16(q, dims)
        e16 = screened_error(rmax, qs16, dims)
        stages.append(("binary16", screen16_values(Xh, qh16), lambda s, e=e16: np.full(s.shape, e, F)))
        if int8_kept:
            qh8, ql8, s_q, a_q = query8(q, dsc, mx8, dims)
            vals = screen8_values(q8, s_r, qh8, ql8, s_q)
            with np.errstate(invalid="ignore", over="ignore"):
                stages.append(("int8", vals, lambda s, a=a_q: (a * s_r + F(1.3e-7) * np.abs(s)).astype(F)))
        for stage, values, e_of in stages:
            for order, s in values.items():
                lo, hi, e = interval(metric, s, e_of(s), qn, xn)
                # screened: a finite value and bounds that are not NaN (the selection sends anything else to the exact path)
                fin = (np.abs(s) <= F(3.0e38)) & ~np.isnan(lo) & ~np.isnan(hi)
                with np.errstate(invalid="ignore"):
                    ok = (lo <= d_ref) & (d_ref <= hi)
                bad = fin & ~ok
                assert not bad.any(), (name, dims, stage, order, np.nonzero(bad)[0][:5], s[bad][:3], r_ref[bad][:3], e[bad][:3])
                checked += int(fin.sum())
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.abs(s.astype(np.float64) - r_ref) / e.astype(np.float64)
                sel = fin & np.isfinite(ratio) & np.isfinite(r_ref)
                if sel.any():
                    worst[stage] = max(worst[stage], float(ratio[sel].max()))
            # what must not be screened is recognised: a value beyond binary16's range, an inf row, a tiny row's E
            if name == "beyond 65504":
                assert not np.isfinite(values["exact"][4]) and not np.isfinite(values["lanes"][4]), stage
                if stage == "binary16":  # the inf row makes the dataset-wide maxima NaN: nothing is screened on this copy
                    assert not np.isfinite(values["exact"][3]) and np.isnan(e16), stage
            if name == "tiny rows":
                if stage == "binary16":
                    assert np.isinf(e16)  # the dataset-wide maxima are inf: every candidate survives
                else:
                    assert np.isinf(s_r[0]) and not np.isfinite(values["exact"][0]) and np.isfinite(s_r[1])
    assert name in ("beyond 65504", "tiny rows") or checked > 0
    WORST[(name, dims, metric)] = worst
    print(f"[bound] {name:26s} dims {dims:5d} {'cosine' if metric == O.COSINE else 'dot':6s} max |s - r| / E: "
          f"binary16 {worst['binary16']:.3g}  int8 {worst['int8']:.3g}")
