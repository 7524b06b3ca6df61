"""The judge of the bf16 device tests (tests/bf16_judge.py) held to its own claims, without a GPU: `rne` is torch's bfloat16 conversion,
ties of both parities included; every case tests/test_bf16_edges_gpu.py runs meets the share conditions of its family and stays below
2^24 (the builders assert both); the int64 result equals a float32 evaluation in ascending, descending and a random order of k;
and every mutation of the model is caught by the family meant to catch it."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import bf16_judge as J
from tests import test_bf16_edges_gpu as E


def test_rne_is_torch_bfloat16_conversion():
    rng = np.random.default_rng(1)
    ties_even = np.float32([1.0 + 2.0 ** -8, 257.0, 513.0 + 1.0, 1026.0])            # ..0|1000: down to even
    ties_odd = np.float32([1.0 + 2.0 ** -7 + 2.0 ** -8, 259.0, 518.0 + 4.0, 1052.0])
    beside = np.concatenate([np.nextafter(t, np.float32(0)) for t in (ties_even, ties_odd)] +
                            [np.nextafter(t, np.float32(np.inf)) for t in (ties_even, ties_odd)])
    big = np.float32([np.finfo(np.float32).max, 3.3895314e38, 2.0 ** 127, -np.finfo(np.float32).max])   # (the largest fp32 rounds to inf in both)
    rnd = ((1.0 + rng.random(200000)) * np.exp2(rng.integers(-100, 100, 200000)) * rng.choice([-1.0, 1.0], 200000)).astype(np.float32)
    ints = rng.integers(-(1 << 24) + 1, 1 << 24, 200000).astype(np.float32)
    v = np.concatenate([ties_even, -ties_even, ties_odd, -ties_odd, beside, -beside, np.float32([0.0, -0.0]), big, rnd, ints])
    want = torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()
    with np.errstate(over="ignore"):
        got = J.bf16_rne(v)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.signbit(J.bf16_rne(np.float32([-0.0])))[0]
    assert J.rne(np.int64([257, 259, 258, 1026, 1030, 1052])).tolist() == [256, 260, 258, 1024, 1032, 1056]
    # the classifier of the share conditions, on the same numbers
    s = J.shares(np.int64([257, 259, 256, 513]))
    assert (s["tie"], s["down"], s["up"], s["inexact"]) == (0.5, 0.25, 0.25, 0.25)
    # RNE commutes with the ReLU (monotone, keeps the sign): "rounding before the ReLU" IS the device's expression and cannot differ
    x = rng.integers(-3000, 3000, 100000)
    np.testing.assert_array_equal(np.maximum(J.rne(x), 0), J.rne(np.maximum(x, 0)))


def test_mutation_roundings_are_what_they_say():
    v = np.int64([257, 259, 258, 511, 1030, -257, -259])
    assert J.rtz(v).tolist() == [256, 258, 258, 510, 1024, -256, -258]
    assert J.rhu(v).tolist() == [258, 260, 258, 512, 1032, -258, -260]


_CASES = list(E.all_cases())


@pytest.mark.parametrize("i", range(len(_CASES)), ids=[f"{f.__name__}-{'-'.join(map(str, a))}".replace(" ", "") for f, a in _CASES])
def test_every_gpu_case_meets_its_family_conditions(i):
    """The builders assert the share conditions (>= 5 % ties, >= 1 % of each parity, >= 25 % inexact non-ties) on the values their
    family rounds, the 8-bit limit of family S, and -- inside J.forward -- sum |w||h| + |b| < 2^24 per output element."""
    build, args = _CASES[i]
    build(*args)




ORDER_CASES = [("S", (40, 70), 0), ("T", (134, 128, 128, 128), 1), ("T", (40, 128, 96), 0), ("W", (134, 128, 128, 128), 0), ("W", (67, 96, 128), 1),
               ("S", (515, 64), 0)]


@pytest.mark.parametrize("family,widths,target", ORDER_CASES)
def test_forward_is_independent_of_the_summation_order(family, widths, target):
    rng = np.random.default_rng(len(widths) + target + ord(family))
    layers, make_x = J.lattice(family, widths, target, rng, last_signed=False)
    x = make_x((2,), 9)
    relu = [True] * len(layers)
    ref = J.forward(layers, x, relu)
    for order in ("asc", "desc", "perm"):
        got = J.forward_f32(layers, x, relu, order=order, rng=rng)
        for r, g in zip(ref, got):
            np.testing.assert_array_equal(g, r.astype(np.float32), err_msg=order)
    # ... and with the on-load transform
    xg, a, b = J.affine_case(rng, (2,), widths[0], 9)
    lay = J.dense_small_layer(rng, widths[0], 32)
    ref = J.forward([lay], xg, [False], ab=[(a, b)])[0]
    for order in ("asc", "desc", "perm"):
        np.testing.assert_array_equal(J.forward_f32([lay], xg, [False], ab=[(a, b)], order=order, rng=rng)[0], ref.astype(np.float32))


def _differs(a, b):
    return float((np.asarray(a) != np.asarray(b)).mean())


def _with(**kw):
    return dataclasses.replace(J.CONTRACT, **kw)


@pytest.mark.parametrize("c0,l,B", E.CHAIN[:2])
@pytest.mark.parametrize("target", [0, 1, 2])
def test_handover_mutations_are_caught_by_family_T(c0, l, B, target):
    """Truncation, round-half-up and no rounding at the hand-over: family T.  (Behind layer 3 the hand-over is the bf16 store.)"""
    layers, x, outs = E.chain_case("T", c0, l, B, target)
    ref = J.rne(outs[2])
    for name, f in (("truncation", J.rtz), ("round half up", J.rhu), ("no rounding", J.ident)):
        bad = J.forward(layers, x, [True] * 3, model=_with(handover=f))
        assert _differs(f(bad[2]), ref) > 0.01, (name, target)
    # round-half-up differs from RNE exactly on the ties that go down to even; truncation on every value that rounds up
    s = J.shares(outs[target])
    assert s["down"] >= 0.01 and s["up"] >= 0.01


@pytest.mark.parametrize("cin,cout,L,B", E.DENSE)
def test_affine_mutations_are_caught_by_family_G(cin, cout, L, B):
    """The ReLU on the wrong side of the transform (bf16(fma(a, relu(x), b)): with a negative a the contract kills what this keeps --
    rounding before or after the ReLU itself is the same number, see test_rne_is_torch_bfloat16_conversion) and the rounding in
    front of instead of behind fma(a, x, b) (the operand left as relu(a bf16(x) + b)): family G."""
    lay, x, ab, ref = E.affine_dense_case(cin, cout, L, B)
    relu_first = J.forward([lay], x, [False], ab=[ab], model=_with(affine=lambda a, h, b: J.rne(a * np.maximum(h, 0) + b)))[0]
    assert _differs(relu_first, ref) > 0.05
    round_first = J.forward([lay], x, [False], ab=[ab], model=_with(affine=lambda a, h, b: np.maximum(a * J.rne(h) + b, 0)))[0]
    assert _differs(round_first, ref) > 0.05
    for f in (J.rtz, J.rhu):
        assert _differs(J.forward([lay], x, [False], ab=[ab], model=_with(affine=lambda a, h, b, f=f: f(np.maximum(a * h + b, 0))))[0], ref) > 0.01


@pytest.mark.parametrize("cin,cout,L,B", E.DENSE)
def test_pack_and_load_mutations_are_caught_by_family_W(cin, cout, L, B):
    """Weights truncated at pack time (and: rounded half up, not rounded), the fp32 input truncated at load: family W."""
    lay, x, ref = E.dense_case("W", cin, cout, L, B, False)
    for f in (J.rtz, J.rhu, J.ident):
        assert _differs(J.forward([lay], x, [False], model=_with(pack=f))[0], ref) > 0.05
        assert _differs(J.forward([lay], x, [False], model=_with(load=f))[0], ref) > 0.05


@pytest.mark.parametrize("cin,cout,L,B", E.DENSE)
def test_data_movement_mutations_are_caught_by_family_S(cin, cout, L, B):
    """Two channels of a 16-slot block swapped, the last k-step dropped, the last ragged position replaced by its neighbour: family S."""
    lay, x, ref = E.dense_case("S", cin, cout, L, B, False)
    hits = 0
    for blk in range((cin + 15) // 16):
        k0, k1 = 16 * blk + 4, 16 * blk + 8                                  # slots 4 and 8 of the block: what a wrong permutation exchanges
        if k1 < cin:
            hits += _differs(J.forward([lay], J.swap_channels(x, k0, k1), [False])[0], ref) > 0
    assert hits == sum(16 * blk + 8 < cin for blk in range((cin + 15) // 16)), "every block's swap changes some output"
    assert _differs(J.forward([lay], J.drop_last_kstep(x), [False])[0], ref) > 0
    assert _differs(J.repeat_neighbour(ref)[..., -1], ref[..., -1]) > 0.5


@pytest.mark.parametrize("cfeat,chans,K,B,N,M", [E.SA[0], E.SA[3], E.SA[7]])
def test_pool_mutation_is_caught_by_family_S(cfeat, chans, K, B, N, M):
    """A max-pool that skips the last neighbour: family S of the SA scale (random neighbour lists; the padded lists repeat their
    FIRST entry, so the last slot of an unpadded list is a neighbour of its own)."""
    layers, feat, xyz_cn, new_xyz, idx, ref = E.sa_case("S", cfeat, chans, K, B, N, M, 0)
    pts = np.concatenate([feat, np.round(xyz_cn * 64)], axis=1).astype(np.int64) if cfeat else np.round(xyz_cn * 64).astype(np.int64)
    g = np.stack([pts[b][:, idx[b]] for b in range(B)])
    g[:, cfeat:] -= np.moveaxis(np.round(new_xyz * 64).astype(np.int64), 2, 1)[:, :, :, None]
    out3 = J.forward(layers, g.reshape(B, cfeat + 3, M * K), [True] * 3)[2]
    np.testing.assert_array_equal(J.pool(out3, K), ref)
    assert _differs(J.pool(out3, K, skip_last=True), ref) > 0
