"""The certified screens of the forest build, restated in numpy and checked against the ORACLE's f32 margins (no GPU).

The build only uses the sign of a margin (`D::side`, src/distance/mod.rs:103-110).  The device decides it from a coarse
copy of the row and of the normal — int8 first (arroy_amd/csrc/forest.hip: k_shadow_rows8 / k_forest_shadow_normals8 /
stage 0 of k_forest_screen_node), binary16 second (screen_device.h) — whenever |screen value| exceeds a bound E on its
distance to the reference's f32 margin:

    |s - r| <= |n - n~||x~| + |n||x - x~| + gamma_s |n~||x~| + gamma_r |n||x|        (Cauchy-Schwarz, measured norms)

This test rebuilds both copies and both bounds with float32 arithmetic as the kernels do, takes the reference margin r from
the oracle (the restated AVX order), and asserts on several data distributions that a decided pair never has the wrong
sign — the property the GPU tests check under AH_SCREEN_VERIFY=1, here without a GPU — and that the stages decide the share
of the pairs DESIGN.md quotes for the benchmark data."""
import numpy as np
import pytest

from oracle import oracle as O

F = np.float32
UP = lambda pitch: F(1.0) + F(pitch + 64) * F(1.2e-7)  # noqa: E731  (the kernels' round-up factor for measured norms)


def norm_up(v, pitch):
    return np.sqrt((v.astype(F) ** 2).sum(axis=-1, dtype=F)).astype(F) * UP(pitch)


def gamma_r(dims):
    return F(4.0 * (dims // 32 + 6.0 + 62.0) * 5.9604645e-8)


TINY = F(2.0 ** -40)  # kTinyBits of forest.hip: rows below it are never decided by a screen


def dim_scales(X):
    """k_col_maxabs + k_dim_scales: one power of two >= the largest |x_i| of every column (1 for empty columns)."""
    m = np.abs(X).max(axis=0).astype(F)
    d = np.ones_like(m)
    ok = (m > 0) & np.isfinite(m)
    mant, exp = np.frexp(m[ok])              # m = mant 2^exp, mant in [0.5, 1)
    p = np.where(mant == 0.5, exp - 1, exp)  # a power of two stays itself, anything else rounds up
    d[ok] = np.where((p >= -63) & (p <= 63), np.ldexp(F(1.0), p), F(1.0)).astype(F)
    return d


def stage_int8_lo(X, nv, dims, bias=None):
    """Stage 1 of the node-major screen: stage 0 plus the rows' second int8 digit (k_shadow_rows8's rows8_lo)."""
    return stage_int8(X, nv, dims, bias=bias, second_digit=True)


def stage_int8(X, nv, dims, bias=None, second_digit=False):
    """(screen value, bound) of every row against `nv`, as stage 0 of k_forest_screen_node computes them: rows scaled per
    dimension (powers of two) and per row, the normal in two int8 digits; cosine (bias None) in units of the row's scale,
    Euclidean / Manhattan in real units."""
    pitch8 = (dims + 127) // 128 * 128
    d = dim_scales(X)
    Y = (X / d).astype(F)                                   # exact
    m = np.abs(Y).max(axis=1).astype(F)
    xm = np.abs(X).max(axis=1).astype(F)
    ok = (m >= TINY) & (xm >= TINY) & np.isfinite(m) & np.isfinite(xm)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(ok, m / F(127.0), F(0.0)).astype(F)[:, None]
        inv = np.where(ok, F(127.0) / m, F(0.0)).astype(F)[:, None]
    if not ok.any():  # the device keeps no int8 copy of such a dataset (ensure_screen8: max |q| == 0)
        return np.zeros(len(X), dtype=F), np.full(len(X), F(np.inf), dtype=F)
    q = np.clip(np.rint(Y * inv), -127, 127).astype(np.int32)
    q2 = np.zeros_like(q)
    if second_digit:  # q2 = round((y / s_r - q) 256), the value the device rebuilds is (q + q2 / 256) s_r
        q2 = np.clip(np.rint(((Y * inv).astype(F) - q.astype(F)) * F(256.0)), -127, 127).astype(np.int32)
    v = (q.astype(F) + q2.astype(F) * F(0.00390625)).astype(F)
    z = (v * scale).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        up = UP(pitch8) * F(1.000001)
        a8 = (norm_up(v, pitch8) * F(1.000001))[ok].max()
        b8 = ((norm_up(Y - z, pitch8) * F(1.000001) + F(128.0) * scale[:, 0] * F(6.0e-8) * np.sqrt(F(pitch8))) / scale[:, 0] * F(1.000001))[ok].max()
        c8 = (norm_up(X, pitch8) * F(1.000001) / scale[:, 0] * F(1.000001))[ok].max()
    nd = (nv * d).astype(F)                                 # exact
    mn = F(np.abs(nd).max())
    sn, invn = F(mn / F(127.0)), F(F(127.0) / mn)
    t = (nd * invn).astype(F)
    qh = np.clip(np.rint(t), -127, 127).astype(np.int32)
    ql = np.clip(np.rint((t - qh.astype(F)) * F(256.0)), -127, 127).astype(np.int32)
    yn = ((qh.astype(F) + ql.astype(F) * F(0.00390625)) * sn).astype(F)
    an, cn, cn0 = norm_up(yn, pitch8), norm_up(nd, pitch8), norm_up(nv, pitch8)
    bn = norm_up(nd - yn, pitch8) + F(128.0) * sn * F(6.0e-8) * np.sqrt(F(pitch8))
    S = ((q @ qh).astype(F) + (q @ ql).astype(F) * F(0.00390625)).astype(F)  # exact integer dots
    if second_digit:
        S = (S + ((q2 @ qh).astype(F) + (q2 @ ql).astype(F) * F(0.00390625)).astype(F) * F(0.00390625)).astype(F)
    S = (S * sn).astype(F)
    e = bn * a8 + cn * b8 + F(2.0e-6) * (an * a8) + gamma_r(dims) * (cn0 * c8)
    if bias is None:
        return S.astype(F), np.full(len(X), F(e * F(1.002) + F(1e-30)), dtype=F)
    s_row = np.where(ok, scale[:, 0], F(np.inf)).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        sd = (S * s_row).astype(F)
        e = (e * s_row * F(1.000001) + F(1.2e-7) * np.abs(sd)).astype(F)
        mval = (F(bias) + sd).astype(F)
        e = (e + F(2.4e-7) * (np.abs(F(bias)) + np.abs(sd) + e)).astype(F)
        e = (e * F(1.002) + F(1e-30)).astype(F)
    return mval, e


def stage_binary16(X, nv, dims, bias=None, gamma_s=None):
    """(screen value, bound) of the binary16 stage.  gamma_s: None = the row-order kernels' (screen_device.h), or the value of
    another product over the same copies (the dense MFMA screen's, forest.hip: `da.gamma_s`)."""
    hpitch = (dims + 63) // 64 * 64
    def shadow(v):
        h = v.astype(np.float16)
        h[np.abs(h.astype(F)) < F(6.103515625e-05)] = 0  # binary16 subnormals become 0
        return h.astype(F)
    Xh, nh = shadow(X), shadow(nv)
    ax, bx, cx = norm_up(Xh, hpitch), norm_up(X - Xh, hpitch), norm_up(X, hpitch)
    an, bn, cn = norm_up(nh, hpitch), norm_up(nv - nh, hpitch), norm_up(nv, hpitch)
    xm = np.abs(X).max(axis=1)
    tiny = (xm != 0) & (xm < TINY)  # k_shadow_rows: f32 squares of such rows underflow -> stats +inf -> never decided
    ax, bx, cx = (np.where(tiny, F(np.inf), v).astype(F) for v in (ax, bx, cx))
    gamma_s = F(4.0 * (2.0 * (hpitch // 16) + 8.0) * 5.9604645e-8) if gamma_s is None else F(gamma_s)
    s = (Xh.astype(np.float64) @ nh.astype(np.float64)).astype(F)  # any accumulation order: covered by gamma_s
    with np.errstate(invalid="ignore", over="ignore"):
        e = (bn * ax + cn * bx + gamma_s * (an * ax) + gamma_r(dims) * (cn * cx)).astype(F)
        if bias is not None:  # Euclidean / Manhattan: r = fl(bias + fl_ref(dot)), screen_decides
            e = (e + F(2.4e-7) * (np.abs(F(bias)) + np.abs(s) + e)).astype(F)
            s = (F(bias) + s).astype(F)
        e = (e * F(1.002) + F(1e-30)).astype(F)
    return s, e


def cases():
    rng = np.random.default_rng(11)
    yield "uniform-768 (the benchmark rows)", rng.uniform(-1, 1, (4000, 768)).astype(F)
    yield "gaussian-768", rng.standard_normal((4000, 768)).astype(F)
    yield "gaussian-96 x 1e-3", (rng.standard_normal((4000, 96)) * 1e-3).astype(F)
    yield "uniform-200 shifted", (rng.uniform(-1, 1, (4000, 200)) + 5.0).astype(F)
    yield "mixed norms-256", (rng.standard_normal((4000, 256)) * rng.uniform(0.01, 3.0, (4000, 1))).astype(F)
    out = rng.standard_normal((4000, 768)).astype(F)
    out[:, 13::97] *= F(20.0)  # a few outlier dimensions x 20 (AH_SYNTH_NORMAL_OUTLIERS)
    yield "gaussian-768 with outlier dimensions", out
    yield "irwin-hall-768 (AH_SYNTH_NORMAL)", O.synth(42, 2, 4000, 768)


@pytest.mark.parametrize("name,X", list(cases()), ids=[c[0] for c in cases()])
def test_a_decided_pair_never_has_the_wrong_sign(name, X):
    dims = X.shape[1]
    data = O.Data(O.COSINE, X)
    rng = np.random.default_rng(dims)
    decided8 = decided8b = decided16 = total = 0
    for _ in range(6):
        nv, nh = data.create_split(rng.choice(len(X), 12, replace=False).astype(np.uint32))  # a real two-means normal
        nv = np.asarray(nv, dtype=F)[:dims]
        _sides, _n_left, r = data.split_sides(nv, nh)  # reference f32 margins (cosine: the dot in the AVX order)
        for stage in (stage_int8, stage_int8_lo, stage_binary16):
            s, e = stage(X, nv, dims)
            dec = np.abs(s) > e
            assert np.all(np.signbit(s[dec]) == np.signbit(r[dec])), f"{name}: {stage.__name__} decided a pair wrongly"
            assert np.all(r[dec] != 0)
            if stage is stage_int8:
                decided8 += int(dec.sum())
            elif stage is stage_int8_lo:
                decided8b += int(dec.sum())
            else:
                decided16 += int(dec.sum())
        total += len(X)
    if name.startswith("uniform-768"):
        assert decided8 > 0.85 * total, decided8 / total    # ~90 % decided by the int8 stage
        assert decided16 > 0.985 * total, decided16 / total  # §2.2: ~1 % fall back to f32
        assert decided8b > 0.995 * total, decided8b / total  # the rows' second digit: 16-bit operands beat binary16's 11
    if name.startswith(("gaussian-768", "irwin-hall-768")):
        # one scale per row (+ one power of two per dimension): Gaussian rows and outlier dimensions quantise as well as
        # uniform rows (round 2, one scale per dataset: the copy was dropped for N(0,1) data)
        assert decided8 > 0.70 * total, (name, decided8 / total)  # measured: 0.77 gaussian, 0.73 with outlier dimensions, 0.81 Irwin-Hall


@pytest.mark.parametrize("scale", [1.0, 1e-6, 7e-24, 3e-31, 1e20])
def test_euclidean_bias_never_decides_alone(scale):
    """Round-2 advisor finding: with rows at 1e-23 the f32 sums of squares behind the measured norms underflow, the bound
    collapsed to 0 and sign(bias) alone decided Euclidean margins — wrongly for half the pairs.  Rows below 2^-40 now carry
    +inf stats (binary16 stage) / an infinite scale (int8 stage) and are never decided; everything else stays sound."""
    rng = np.random.default_rng(5)
    dims, n = 96, 4000
    X = (rng.standard_normal((n, dims)) * scale).astype(F)
    data = O.Data(O.EUCLIDEAN, X)
    wrong = decided = 0
    for _ in range(6):
        nv, nh = data.create_split(rng.choice(n, 12, replace=False).astype(np.uint32))
        nv = np.asarray(nv, dtype=F)[:dims]
        bias = F(np.asarray(nh, dtype=F).ravel()[0])
        _sides, _n_left, r = data.split_sides(nv, nh)  # reference: fl(bias + dot), AVX order
        for stage in (stage_int8, stage_int8_lo, stage_binary16):
            m, e = stage(X, nv, dims, bias=bias)
            with np.errstate(invalid="ignore"):
                dec = np.abs(m) > e
            wrong += int((np.signbit(m[dec]) != np.signbit(r[dec])).sum())
            decided += int(dec.sum())
    assert wrong == 0, (scale, wrong, decided)
    if scale < 1e-12:
        assert decided == 0  # tiny rows take the reference arithmetic
    if scale == 1.0:
        assert decided > 0.5 * 12 * n


def _rtz32(x64):
    """float64 -> float32 rounded toward zero (a truncating adder)."""
    y = np.float32(x64)
    if abs(float(y)) > abs(float(x64)):
        y = np.nextafter(y, np.float32(0.0))
    return y


def test_gamma_of_the_dense_product_covers_any_order_and_a_truncating_adder():
    """The dense MFMA screen (dense_device.h) sums the hpitch exact binary16 products of a pair in one f32 chain whose order
    and rounding mode the matrix unit does not document.  Its gamma_s = 2 (hpitch + hpitch / 16 + 16) 2^-23 must cover
    |sum_f32 - sum_exact| / sum |x~_i n~_i| for sequential, reversed, shuffled and 16-wide-blocked orders, with round-to-
    nearest and with truncation after every addition."""
    rng = np.random.default_rng(3)
    hpitch = 768
    gamma = 2.0 * (hpitch + hpitch / 16 + 16.0) * 1.1920929e-7
    worst = 0.0
    for _ in range(12):
        x = rng.uniform(-1, 1, hpitch).astype(np.float16).astype(np.float64)
        n = (rng.standard_normal(hpitch) / np.sqrt(hpitch)).astype(np.float16).astype(np.float64)
        p = x * n  # exact in float64 (and in f32: 11-bit x 11-bit significands)
        exact, scale = p.sum(), np.abs(p).sum()
        orders = [np.arange(hpitch), np.arange(hpitch)[::-1], rng.permutation(hpitch)]
        for order in orders:
            acc_rn, acc_tz = np.float32(0.0), np.float32(0.0)
            for v in p[order]:
                acc_rn = np.float32(np.float64(acc_rn) + v)        # round to nearest after every addition
                acc_tz = _rtz32(np.float64(acc_tz) + v)             # truncate after every addition
            blocked = np.float32(0.0)
            for b in range(0, hpitch, 16):                           # a 16-wide step summed exactly, then one rounding
                blocked = _rtz32(np.float64(blocked) + p[order][b:b + 16].sum())
            for got in (acc_rn, acc_tz, blocked):
                worst = max(worst, abs(float(got) - exact) / scale)
    assert worst < gamma / 2, (worst, gamma)  # at least a factor 2 of head-room on these inputs
