"""The int8 stages of the node-major screen for DotProduct (AH_SCREEN8_DOT; forest.hip: screen8_decides<AH_DOT_PRODUCT>) restated
in numpy, float32 operation by operation, against the ORACLE's margins r = fl(fl_ref(<n, x>) + fl(h0 e_x)) (no GPU): a decided
pair has the sign of r; tiny and non-finite rows are never decided; the all-zero row's m = fl(h0 e_x) is r itself."""
import numpy as np
import pytest

from oracle import oracle as O
from test_screen_bound_cpu import F, TINY, dim_scales, gamma_r

N, ZERO, TINY_ROW, INF_ROW = 3000, 5, 6, 7
P256 = F(0.00390625)


def digits(v, inv):  # two int8 digits of v * inv, both clamped to +-127
    t = (v * inv).astype(F)
    q = np.clip(np.rint(t), -127, 127).astype(F)
    return q, np.clip(np.rint((t - q) * F(256.0)), -127, 127).astype(F)


def norm(v):
    return np.sqrt((v.astype(F) ** 2).sum(axis=-1, dtype=F)).astype(F)


def dot8_stage(X, ex, nv, h0, lo):
    """(m, E) of every row against the normal (nv, h0): stage 0, or stage 1 (`lo`: with the rows' second digit)."""
    dims = X.shape[1]
    pitch, pitch8 = (dims + 31) // 32 * 32, (dims + 127) // 128 * 128
    d = dim_scales(X)
    with np.errstate(all="ignore"):
        Y = (X / d).astype(F)  # exact
        my, mx = np.abs(Y).max(axis=1), np.abs(X).max(axis=1)
        ok = (my >= TINY) & (mx >= TINY) & np.isfinite(my) & np.isfinite(mx)
        s = np.where(ok, my / F(127.0), F(0.0)).astype(F)
        Yq = np.where(ok[:, None], Y, F(0.0))  # rows that are not usable store q = 0
        q, q2 = digits(Yq, np.where(ok, F(127.0) / my, F(0.0)).astype(F)[:, None])
        v = (q + q2 * P256).astype(F) if lo else q
        # k_shadow_rows8: dataset-wide maxima over the usable rows, in units of the row's scale, rounded up
        up = (F(1.0) + F(pitch + 64) * F(1.2e-7)) * F(1.000001)
        a8 = (norm(v) * up)[ok].max()
        b8 = ((norm(Yq - v * s[:, None]) * up + F(128.0 if lo else 127.0) * s * F(6.0e-8) * np.sqrt(F(pitch))) / s * F(1.000001))[ok].max()
        c8 = (norm(X) * up / s * F(1.000001))[ok].max()
        s_row = np.where(ok, s, np.where(mx == 0, F(0.0), F(np.inf))).astype(F)
        # k_forest_shadow_normals8: the normal scaled per dimension, two digits, measured norms
        nd = (nv * d).astype(F)
        mn = F(np.abs(nd).max())
        n_ok = bool(mn >= TINY and np.isfinite(mn))
        sn = F(mn / F(127.0)) if n_ok else F(0.0)
        qh, ql = digits(nd, F(F(127.0) / mn) if n_ok else F(0.0))
        yn, upn = ((qh + ql * P256) * sn).astype(F), F(1.0) + F(pitch8 + 64) * F(1.2e-7)
        bn = norm(nd - yn) * upn + F(128.0) * sn * F(6.0e-8) * np.sqrt(F(pitch8)) if n_ok else F(np.inf)
        S = ((q @ qh).astype(F) + (q @ ql).astype(F) * P256).astype(F)  # exact integer dots
        if lo:
            S = (S + ((q2 @ qh).astype(F) + (q2 @ ql).astype(F) * P256).astype(F) * P256).astype(F)
        # screen8_decides<AH_DOT_PRODUCT>
        e = F(bn * a8 + norm(nd) * upn * b8 + F(2.0e-6) * (norm(yn) * upn * a8) + gamma_r(dims) * (norm(nv) * upn * c8))
        sd, p = ((S * sn).astype(F) * s_row).astype(F), (F(h0) * ex).astype(F)
        e = (e * s_row * F(1.000001) + F(1.2e-7) * np.abs(sd)).astype(F)
        e = (e + F(2.4e-7) * (F(2.0) * np.abs(p) + np.abs(sd) + e)).astype(F)
        return (sd + p).astype(F), (e * F(1.002) + F(1e-30)).astype(F)


# (the fourth kind: the special rows without the inf, which makes max_norm and so every row's e_x infinite — nothing is decided)
@pytest.mark.parametrize("dims", [40, 768])
@pytest.mark.parametrize("kind", ["uniform", "norms 1e-3..1e3", "special rows", "special rows, finite"])
def test_a_decided_dot_product_pair_has_the_sign_of_the_oracle_margin(kind, dims):
    rng = np.random.default_rng(dims + len(kind))
    X = rng.uniform(-1, 1, (N, dims)).astype(F)
    if kind.startswith("norms"):  # after the preprocessing h0 e_x dominates the margins of the short rows
        X = (X * 10.0 ** rng.uniform(-3, 3, (N, 1))).astype(F)
    if kind.startswith("special"):
        X[ZERO], X[TINY_ROW] = 0.0, F(1e-30)
        X[INF_ROW, 3] = np.inf if kind == "special rows" else X[INF_ROW, 3]
    data = O.Data(O.DOT_PRODUCT, X)
    data.preprocess_dot()
    ex = data.headers[:, 0].copy()
    decided = [0, 0]
    for _ in range(6):
        nv, nh = data.create_split(rng.choice(np.arange(8, N), 12, replace=False).astype(np.uint32))  # a real two-means normal
        _sides, _n_left, r = data.split_sides(nv, nh)  # ao_margin of every row
        for stage in (0, 1):
            m, e = dot8_stage(X, ex, nv.view(F), nh[0], lo=stage == 1)
            with np.errstate(invalid="ignore"):
                dec = np.abs(m) > e
            assert np.all(np.signbit(m[dec]) == np.signbit(r[dec])) and np.all(r[dec] != 0), f"stage {stage} decided a pair wrongly"
            if kind.startswith("special"):
                assert not dec[TINY_ROW] and (kind != "special rows" or not dec[INF_ROW]), "a tiny or non-finite row was decided"
            if kind == "special rows, finite":
                assert dec[ZERO] and m[ZERO] == r[ZERO]
            decided[stage] += int(dec.sum())
    print(f"{kind}, {dims} dims: stage 0 decides {decided[0] / (6 * N):.4f} of the pairs, stage 1 {decided[1] / (6 * N):.4f}")
