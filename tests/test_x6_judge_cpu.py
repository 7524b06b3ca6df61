"""The judge of the f32x6 device tests (tests/x6_judge.py) held to its own claims, without a GPU: the split is exact, probe pairs see
every kept product at >= 32 * 2^-24 |w x| while any summation order of the six stays within 8 * 2^-24, the integer lattices stay
inside the range where fp32 sums are order-free, and every mutation of the model (one kept product dropped, pieces 1 and 2
swapped on either side) is caught by the family meant to catch it."""
import numpy as np
import pytest

from tests import x6_judge as J

U = J.U


def _random_fp32(rng, n):
    """Random mantissas over the exponents the device tests use, both signs, plus the edges of the split (ties, all-ones mantissas)."""
    v = ((1.0 + rng.random(n)) * np.exp2(rng.integers(-100, 100, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    edges = np.float32([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 2.0 - 2.0 ** -23, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -16 + 2.0 ** -23,
                        1.00390625, 1.01171875, -1.0 - 2.0 ** -8 - 2.0 ** -16 - 2.0 ** -23])
    return np.concatenate([v, edges, edges * np.float32(2.0 ** 90), edges * np.float32(2.0 ** -90)])


def test_split3_is_exact_and_bf16():
    rng = np.random.default_rng(1)
    v = _random_fp32(rng, 200000)
    v0, v1, v2 = J.split3(v)
    for p in (v0, v1, v2):
        assert ((p.view(np.uint32) & 0xFFFF) == 0).all()                  # bf16 values
    assert (v0.astype(np.float64) + v1.astype(np.float64) + v2.astype(np.float64) == v.astype(np.float64)).all()
    # RNE: each piece is within half a bf16 ulp of what it rounds
    assert (np.abs(v.astype(np.float64) - v0) <= 2.0 ** -8 * np.abs(v.astype(np.float64))).all()
    assert (np.abs(v1.astype(np.float64)) <= 2.0 ** -8 * np.abs(v.astype(np.float64)) * (1 + 2.0 ** -7)).all()
    # ties go to even: 1 + 2^-8 -> 1, 1 + 2^-7 + 2^-8 -> 1 + 2^-6
    assert J.bf16_rne(np.float32([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8])).tolist() == [1.0, 1.0 + 2.0 ** -6]


def test_model_of_all_nine_products_is_the_exact_product():
    rng = np.random.default_rng(2)
    w = rng.standard_normal((48, 16)).astype(np.float32)
    x = rng.standard_normal((2, 48, 24)).astype(np.float32)
    b = rng.standard_normal(16).astype(np.float32)
    all_nine = tuple((i, j) for i in range(3) for j in range(3))
    ref = np.einsum("kc,bkl->bcl", w.astype(np.float64), x.astype(np.float64)) + b.astype(np.float64)[None, :, None]
    np.testing.assert_allclose(J.x6_layer_model(w, x, b, all_nine), ref, rtol=0, atol=1e-13)
    # the six kept ones: three products of <= 2^-8 * 2^-16 |w x| (1 + 2^-7) each are missing
    absref = np.einsum("kc,bkl->bcl", np.abs(w).astype(np.float64), np.abs(x).astype(np.float64))
    assert (np.abs(J.x6_layer_model(w, x, b) - ref) <= 3 * (1 + 2.0 ** -7) * U * absref).all()


def test_probe_filter_acceptance_sensitivity_and_worst_order():
    """The figures of the final filter (2^-9.5 and 2^-19, each times 1 + 2^-7), measured here: ~30 % of random mantissas pass; over
    4000 pairs the smallest kept product is >= 32 U |w x| (by construction, see the judge), the float64 model is within 1 U and the
    fp32 sum of the six products in ANY of the 720 orders within 8 U of the exact product."""
    rng = np.random.default_rng(3)
    m = (1.0 + rng.random(100000)).astype(np.float32)
    rate = J.is_probe(m).mean()
    assert 0.2 < rate < 0.45, rate
    w, x = J.probe_values(rng, 4000), J.probe_values(rng, 4000)
    assert J.is_probe(w).all() and J.is_probe(x).all()
    exact = np.abs(w.astype(np.float64) * x.astype(np.float64))
    prods = np.abs(J.six_products(w, x))
    smallest = (prods / exact).min(axis=1) / U
    print("smallest kept product per kind, in U:", dict(zip(J.ALL_SIX, smallest.round(1))))
    assert smallest.min() >= J.PROBE_SENS
    model_err = np.abs(J.six_products(w, x).sum(0) - w.astype(np.float64) * x) / exact / U
    worst = J.worst_order_error(w, x)
    print(f"acceptance {rate:.3f}, float64 model within {model_err.max():.2f} U, worst of 720 fp32 orders {worst:.2f} U")
    assert model_err.max() <= 1.0
    assert worst <= J.PROBE_TOL
    # every single-product drop (and each swap) moves the model by >= 32 U: 4 x the tolerance
    full = J.six_products(w, x).sum(0)
    for drop in J.ALL_SIX:
        keep = tuple(p for p in J.ALL_SIX if p != drop)
        assert (np.abs(J.six_products(w, x, keep).sum(0) - full) / exact).min() >= J.PROBE_SENS * U, drop
    # a swap of pieces 1 and 2 on one side puts w1 x2 (or w2 x1) where w1 x1 belongs: the model moves by |w1 x1| - |w1 x2| >=
    # (1 - 2^-7) |w1 x1| (|x2| <= 2^-8 |x1| / (1 - 2^-8)), and |w1 x1| >= 2^-19 (1 + 2^-7)^2 |w x| by the filter: >= 32 U for EVERY pair
    for swap in (J.SWAP_X12, J.SWAP_W12):
        moved = np.abs(J.six_products(w, x, swap).sum(0) - full) / exact
        assert moved.min() >= J.PROBE_SENS * U, (swap, moved.min() / U)


def test_pow2_perm_passes_a_value_on():
    rng = np.random.default_rng(4)
    for cin, cout in ((128, 128), (64, 96), (196, 128), (128, 2)):
        w, src = J.pow2_perm(rng, cin, cout)
        assert ((w != 0).sum(0) <= 1).all() and ((w != 0).sum(1) <= 1).all()
        assert (w != 0).sum() == min(cin, cout)
        x = J.probe_values(rng, (cin, 5))
        y = J.x6_layer_model(w, x)
        cs = np.nonzero(src >= 0)[0]
        np.testing.assert_array_equal(y[cs], w[src[cs], cs][:, None].astype(np.float64) * x[src[cs]])     # one piece of w: nothing dropped


WIDTHS = [((16, 256), 0), ((176, 512), 0), ((1024, 256), 0), ((131, 128, 128, 128), 0), ((134, 128, 128, 128), 1), ((134, 128, 128, 128), 2),
          ((134, 128, 128, 128, 2), 3), ((128, 196, 256), 0), ((64, 96, 128), 1), ((32, 32, 64), 1)]


@pytest.mark.parametrize("family", "ABC")
@pytest.mark.parametrize("widths,target", WIDTHS)
def test_lattice_is_exact_and_catches_its_mutations(family, widths, target):
    rng = np.random.default_rng(len(widths) * 7 + target + ord(family))
    layers, make_x = J.lattice(family, widths, target, rng)
    x = make_x((2,), 40)
    relu = [True] * (len(layers) - 1) + [False]
    ref = J.lattice_forward(layers, x, relu)                               # asserts sum |w||h| + |b| < 2^24 after every layer
    assert all(np.abs(r).max() < J.LIMIT for r in ref)
    got = J.lattice_forward(layers, x, relu, keep=J.ALL_SIX)
    for r, g in zip(ref, got):
        np.testing.assert_array_equal(g, r.astype(np.float64))            # the three dropped products are exactly zero
    # the non-zeros are where the family says
    tl = layers[target]
    assert ((tl.w != 0).sum(0) == (4 if family == "A" else 2)).all()
    assert all(((lay.w != 0).sum(0) == 1).all() for i, lay in enumerate(layers) if i != target)
    # the target layer reads min(cin, nnz * cout) DIFFERENT input channels: all of them, except where the layer has fewer non-zeros
    # than inputs -- (1024, 256) with two per column reads 512 (there every k slot is family (b)'s to see, not the lattice's)
    assert (tl.w != 0).any(1).sum() == min(tl.cin, tl.rows.size)
    seen = {"A": [(0, 0), (0, 1), (1, 0), (1, 1)], "B": [(0, 0), (0, 1), (0, 2)], "C": [(0, 0), (1, 0), (2, 0)]}[family]
    for drop in seen:
        keep = tuple(p for p in J.ALL_SIX if p != drop)
        bad = J.lattice_forward(layers, x, relu, keep=keep)[-1]
        assert (bad != ref[-1]).mean() > 0.1, (family, drop)
    if family == "A":
        for swap in (J.SWAP_X12, J.SWAP_W12):
            assert (J.lattice_forward(layers, x, relu, keep=swap)[-1] != ref[-1]).mean() > 0.1
    # (B and C hold one piece on one side: a swap of pieces 1 and 2 leaves all their products in place -- family A's to catch)


def test_lattice_pieces_are_what_the_families_claim():
    rng = np.random.default_rng(9)
    for family in "ABC":
        layers, make_x = J.lattice(family, (64, 256), 0, rng)
        w, x = layers[0].w, make_x((1,), 64).astype(np.float32)
        wn, xn = w[w != 0], x
        pw, px = J.split3(wn), J.split3(xn)
        if family == "A":
            assert (pw[1] != 0).all() and (px[1] != 0).all() and (pw[2] == 0).all() and (px[2] == 0).all()
            for v in (np.abs(wn), np.abs(xn)):
                assert (v >= 2 ** 8).all() and (v < 2 ** 12).all() and (v % 2 == 1).all()
        elif family == "B":
            assert (pw[1] == 0).all() and (px[2] != 0).all() and (np.abs(xn) >= 2 ** 16).all() and (np.abs(xn) < 2 ** 20).all() and (np.abs(wn) < 8).all()
        else:
            assert (px[1] == 0).all() and (pw[2] != 0).all() and (np.abs(wn) >= 2 ** 16).all() and (np.abs(wn) < 2 ** 20).all() and (np.abs(xn) < 8).all()


def test_lattice_with_small_outputs_for_statistics():
    """out_max = 256: sum and sum of squares over 128 positions are integers <= 128 * 256^2 = 2^23."""
    rng = np.random.default_rng(10)
    for family in "AB":
        layers, make_x = J.lattice(family, (48, 256), 0, rng, out_max=256)
        y = J.lattice_forward(layers, make_x((2,), 256), [False])[0]
        assert np.abs(y).max() <= 256 and np.abs(y).max() > 16
        assert (y.reshape(2, 256, 2, 128) ** 2).sum(-1).max() < J.LIMIT


def test_rescaling_is_exact_in_the_model():
    """2^a_k on the inputs, 2^-a_k on the weight rows, 2^g_c on the output channels: all products and all sums scale exactly, so
    the model's result scales exactly -- while every piece stays a normal number (asserted range)."""
    rng = np.random.default_rng(11)
    w = (rng.standard_normal((48, 32)) / 7).astype(np.float32)
    x = rng.standard_normal((2, 48, 16)).astype(np.float32)
    b = rng.standard_normal(32).astype(np.float32)
    a, g = rng.integers(-40, 41, 48), rng.integers(-40, 41, 32)
    w2, x2 = J.rescale_in(w, x, a)
    w2, b2 = J.rescale_out(w2, b, g)
    lo, hi = J.piece_range(w, x, b, w2, x2, b2)
    assert lo >= 2.0 ** -120 and hi <= 2.0 ** 100
    for p, q in zip(J.split3(x), J.split3(x2)):
        np.testing.assert_array_equal(p.astype(np.float64) * np.exp2(a)[None, :, None], q)     # the pieces scale one by one
    y1 = J.x6_layer_model(w, x, b) * np.exp2(g)[None, :, None]
    np.testing.assert_allclose(J.x6_layer_model(w2, x2, b2), y1, rtol=1e-15, atol=0)
