"""captra_pose_extrapolate (csrc/pose_motion.hip) through the C ABI and its Python wrapper against the float64 judge of
tests/motion_judge.py.

Both sides compute in double on the same fp32 inputs and round once, so only a difference between two libms (sin, cos, atan2, sqrt's
neighbours) can flip a rounding: trans_next, angle and shift within ONE fp32 ulp of the judge's value; a rotation entry is a sum of
terms of order one, so its bound is absolute, 2^-23.  used / measured1 are exact and every pass-through output is the input's bits
(NaN and Inf included).  The cases keep every angle and shift at least 1e-6 (relative) away from its threshold -- except the shift
that EQUALS max_shift on exactly representable values, which must be used."""
import numpy as np
import pytest

from tests import motion_judge as MJ

SHAPES = [(1, 1), (3, 4), (32, 8), (33, 2)]          # one thread; every (b, p) another motion; 256 threads = four waves; 66: no multiple of 64
_REFS = {}


def _case(B, P, sym, gain, k):
    """A launch's case and the judge's result, built once and shared (never modified)."""
    key = (B, P, sym, gain, k)
    if key not in _REFS:
        case = MJ.make_batch(B, P, sym, gain, k)
        ref = MJ.judge_batch(case)
        MJ.check_batch(case, ref)
        _REFS[key] = (case, ref)
    return _REFS[key]


def _dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _abi(case, device, shape=None, null=(), **over):
    """The C ABI on sentinel-filled outputs -> (err, dict of numpy outputs).  shape = (b, p), null = names of pointers handed over as
    NULL and sym / gain / max_angle / max_shift override the case's (for the refused arguments)."""
    import torch
    from captra_amd import _lib as L
    B, P = case["measured0"].shape
    ins = {k: _dev(case[k], device) for k in ("rot0", "trans0", "rot1", "trans1", "measured0", "verdict")}
    out = dict(rot_next=torch.full((B, P, 3, 3), 7.0, device=device), trans_next=torch.full((B, P, 3), 7.0, device=device),
               measured1=torch.full((B, P), -7, dtype=torch.int32, device=device), used=torch.full((B, P), -7, dtype=torch.int32, device=device),
               angle=torch.full((B, P), -7.0, device=device), shift=torch.full((B, P), -7.0, device=device))
    ptr = lambda name, t: None if name in null else L.ptr(t)      # noqa: E731
    b_, p_ = shape if shape is not None else (B, P)
    get = lambda k: over.get(k, case[k])                            # noqa: E731
    with torch.cuda.device(device):
        err = L.lib().captra_pose_extrapolate(b_, p_, int(get("sym")), *(ptr(k, ins[k]) for k in ("rot0", "trans0", "rot1", "trans1", "measured0", "verdict")),
                                              float(get("gain")), float(get("max_angle")), float(get("max_shift")),
                                              *(ptr(k, out[k]) for k in ("rot_next", "trans_next", "measured1", "used", "angle", "shift")),
                                              L.stream_ptr())
    torch.cuda.synchronize(device)
    return err, {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(got, case, ref, name):
    np.testing.assert_array_equal(got["used"], ref["used"], err_msg=f"{name} used")
    np.testing.assert_array_equal(got["measured1"], ref["measured1"], err_msg=f"{name} measured1")
    for k in ("angle", "shift"):
        assert np.isfinite(got[k]).all(), (name, k)
        err = np.abs(got[k].astype(np.float64) - ref[k])
        assert (err <= np.spacing(np.abs(ref[k]))).all(), (name, k, float(err.max()))
    B, P = ref["used"].shape
    kinds = np.array(case["kinds"]).reshape(B, P)
    for b in range(B):
        for p in range(P):
            tag = (name, b, p, kinds[b, p])
            if not ref["used"][b, p]:                  # the pass-through: rot1 / trans1 bit for bit
                np.testing.assert_array_equal(_bits(got["rot_next"][b, p]), _bits(case["rot1"][b, p]), err_msg=str(tag))
                np.testing.assert_array_equal(_bits(got["trans_next"][b, p]), _bits(case["trans1"][b, p]), err_msg=str(tag))
                continue
            t = ref["trans_next"][b, p]
            assert (np.abs(got["trans_next"][b, p].astype(np.float64) - t) <= np.spacing(np.abs(t))).all(), tag
            if kinds[b, p] == "equal":                 # |v| == 0 exactly: the rotation part is rot1's bits
                np.testing.assert_array_equal(_bits(got["rot_next"][b, p]), _bits(case["rot1"][b, p]), err_msg=str(tag))
            e = np.abs(got["rot_next"][b, p].astype(np.float64) - ref["rot_next"][b, p]).max()
            assert e <= 2.0 ** -23, (tag, e)


@pytest.mark.gpu
@pytest.mark.parametrize("gain", [1.0, 0.5, 0.25])
@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("B,P", SHAPES)
def test_kernel_vs_judge(device, B, P, sym, gain):
    launches = 4 * -(-len(MJ.KINDS) // (B * P))           # every kind at least once, with B P = 1 each with all of k mod 4
    met, worst = set(), 0.0
    for k in range(launches):
        case, ref = _case(B, P, sym, gain, k)
        err, got = _abi(case, device)
        assert err == 0
        _check(got, case, ref, f"B={B} P={P} sym={sym} gain={gain} k={k}")
        met.update(case["kinds"])
        worst = max(worst, float(np.abs(got["rot_next"][ref["used"] == 1].astype(np.float64) - ref["rot_next"][ref["used"] == 1]).max(initial=0.0)))
        edge = np.array(case["kinds"]).reshape(B, P) == "shift_edge"
        assert (got["used"][edge] == 1).all() and (got["shift"][edge] == np.float32(MJ.MAX_SHIFT)).all()
    print(f"B={B} P={P} sym={sym} gain={gain}: {launches} launches, largest rotation entry difference {worst:.2e}")
    assert met == set(MJ.KINDS)


@pytest.mark.gpu
def test_refused_arguments(device):
    case, ref = _case(3, 4, 0, 1.0, 0)
    nan, inf = float("nan"), float("inf")
    refused = [dict(shape=(0, 4)), dict(shape=(-1, 4)), dict(shape=(3, 0)), dict(shape=(3, 9)), dict(sym=2), dict(sym=-1),
               dict(gain=0.0), dict(gain=-0.5), dict(gain=1.0001), dict(gain=nan), dict(max_angle=0.0), dict(max_angle=-1.0),
               dict(max_angle=90.01), dict(max_angle=nan), dict(max_shift=0.0), dict(max_shift=-1.0), dict(max_shift=inf), dict(max_shift=nan)]
    refused += [dict(null=(k,)) for k in ("rot0", "trans0", "rot1", "trans1", "measured0", "rot_next", "trans_next", "measured1", "used", "angle", "shift")]
    for kw in refused:
        err, got = _abi(case, device, **kw)
        assert err == -1, kw
        assert (got["rot_next"] == 7.0).all() and (got["trans_next"] == 7.0).all() and (got["angle"] == -7.0).all() and (got["shift"] == -7.0).all(), kw
        assert (got["used"] == -7).all() and (got["measured1"] == -7).all(), kw
    # the limits themselves are accepted; a smaller launch leaves the rest of the buffers alone
    err, got = _abi(case, device, gain=1.0, max_angle=90.0, shape=(2, 4))
    assert err == 0 and (got["used"][:2] != -7).all() and (got["used"][2:] == -7).all() and (got["rot_next"][2:] == 7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sym", [False, True])
def test_wrapper(device, sym):
    import torch
    from captra_amd.pose_utils.pose_fit import pose_extrapolate
    for k in (1, 2):                                      # verdicts given, verdicts None
        case, ref = _case(33, 2, int(sym), 0.5, k)
        _, got = _abi(case, device)
        d = {key: _dev(case[key], device) for key in ("rot0", "trans0", "rot1", "trans1", "measured0", "verdict")}
        rot, trans, measured, info = pose_extrapolate(d["rot0"], d["trans0"].unsqueeze(-1), d["rot1"], d["trans1"].unsqueeze(-1), d["measured0"], sym,
                                                      case["max_angle"], case["max_shift"], gain=0.5, verdict=d["verdict"])
        assert rot.shape == (33, 2, 3, 3) and trans.shape == (33, 2, 3, 1) and set(info) == {"used", "angle", "shift"}
        assert measured.dtype == torch.int32 and info["used"].dtype == torch.int32 and info["angle"].dtype == torch.float32
        np.testing.assert_array_equal(_bits(rot.cpu().numpy()), _bits(got["rot_next"]))
        np.testing.assert_array_equal(_bits(trans.cpu().numpy()[..., 0]), _bits(got["trans_next"]))
        np.testing.assert_array_equal(measured.cpu().numpy(), got["measured1"])
        for key in ("used", "angle", "shift"):
            np.testing.assert_array_equal(info[key].cpu().numpy(), got[key])
