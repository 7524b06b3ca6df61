"""The shared cloud geometry (captra_amd/geometry.py) through every way PointNet2Msg builds one: whichever way it was made --
precomputed on one stream or two, level 1 first and completed later, with the streamed sampler, inside the level-1 stream kernel,
or left behind by another backbone's forward -- it holds the tensors a forward without a geometry computes for itself, and a
forward that is handed it returns that forward's output.  Bit equality throughout: samplings, neighbour lists and 3-NN weights
depend on the coordinates only, and no launch differs.

B = 2 clouds of N = 1024 points in [-0.4, 0.4]^3: the backbone takes 512 / 128 centres, so this is the smallest power of two that
still samples and leaves every neighbour list partly padded."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N = 2, 1024


def _net(use_xyz, device, seed=4):
    from captra_amd.backbones import PointNet2Msg
    from captra_amd.configs import make_config
    from captra_amd.synthetic import make_state_dict
    net = PointNet2Msg(make_config("1"), 128, use_xyz_feat=use_xyz)
    net.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=seed))
    return net.to(device).eval()


def _cloud(device):
    cn = torch.from_numpy((np.random.default_rng(11).random((B, 3, N), dtype=np.float32) - 0.5) * 0.8).to(device)
    return cn, cn.transpose(1, 2).contiguous()


def _run(net, cn, n3, geom=None):
    """-> (output, the geometry the forward left behind), complete."""
    with torch.no_grad():
        out = net(cn, input_n3=n3, geom=geom)
    torch.cuda.synchronize()
    return out, net.last_geom


def _assert_same_geometry(got, want, tag):
    for name in ("sa1", "sa2"):
        g, w = getattr(got, name), getattr(want, name)
        assert torch.equal(g.new_xyz_n3, w.new_xyz_n3) and torch.equal(g.new_xyz, w.new_xyz), f"{tag}: {name}'s sampling differs"
        assert g.new_xyz_n3.shape == (B, g.new_xyz.shape[2], 3)
        assert len(g.idx_list) == len(w.idx_list) == 3 - (name == "sa2")
        for s, (a, b) in enumerate(zip(g.idx_list, w.idx_list)):
            assert a.dtype == torch.int32 and torch.equal(a, b), f"{tag}: {name}'s neighbour list {s} differs"
    for name in ("fp1", "fp2"):
        for a, b, what in zip(getattr(got, name), getattr(want, name), ("indices", "weights")):
            assert torch.equal(a, b), f"{tag}: {name}'s {what} differ"


@pytest.fixture(scope="module", params=[True, False], ids=["xyz_feat", "bare"])
def plain(request, device):
    """(net, cloud (B,3,N), cloud (B,N,3), out0, g0): a seeded backbone's forward without a geometry.  Left unchanged."""
    net = _net(request.param, device)
    cn, n3 = _cloud(device)
    out0, g0 = _run(net, cn, n3)
    return net, cn, n3, out0, g0


def test_lists_are_partly_padded(plain):
    """The shape is what the docstring says: every list has a centre with fewer neighbours than slots (padded with its first)."""
    g0 = plain[4]
    for lv in (g0.sa1, g0.sa2):
        for idx in lv.idx_list:
            assert bool((idx[:, :, -1] == idx[:, :, 0]).any())


def _precomputed(net, n3):
    return net.precompute_geometry(n3)


def _precomputed_side(net, n3):
    return net.precompute_geometry(n3, side=torch.cuda.Stream())


def _level1_then_rest(net, n3):
    geom = net.precompute_geometry(n3, level1_only=True)
    assert geom.sa2 is None and geom.fp1 is None and geom.fp2 is None and geom.sa1.idx_list is not None
    assert net.precompute_geometry_rest(geom, n3) is geom
    return geom


def _streamed(net, n3):
    geom = net.precompute_geometry_streamed(n3, 4, torch.cuda.Stream())
    assert len(geom.sa1.windows) == 4 and geom.ready is not None
    return geom


@pytest.mark.parametrize("build", [_precomputed, _precomputed_side, _level1_then_rest, _streamed], ids=lambda f: f.__name__.strip("_"))
def test_built_geometry_equals_forwards_own(plain, build):
    net, cn, n3, out0, g0 = plain
    with torch.no_grad():
        geom = build(net, n3)
    assert geom is not None
    torch.cuda.synchronize()
    _assert_same_geometry(geom, g0, build.__name__)
    out, used = _run(net, cn, n3, geom)
    assert torch.equal(out, out0)
    assert used.sa1 is geom.sa1 and used.sa2 is geom.sa2 and used.fp1 is geom.fp1 and used.fp2 is geom.fp2


def test_level1_only_geometry_stays_level1_only(plain):
    """Two backbones may share a level-1-only geometry on two streams: a forward adds its level 2 to its own record, never to the
    shared one."""
    net, cn, n3, out0, g0 = plain
    with torch.no_grad():
        geom = net.precompute_geometry(n3, level1_only=True)
    out, used = _run(net, cn, n3, geom)
    assert geom.sa2 is None and geom.fp1 is None and geom.fp2 is None
    assert torch.equal(out, out0)
    _assert_same_geometry(used, g0, "level 1 only")


def test_second_backbone_takes_the_firsts_geometry(plain, device):
    net, cn, n3, out0, g0 = plain
    other = _net(not net.use_xyz_feat, device, seed=9)
    want, own = _run(other, cn, n3)
    _assert_same_geometry(own, g0, "the other backbone's own")
    got, used = _run(other, cn, n3, g0)
    assert torch.equal(got, want)
    assert used.sa1 is g0.sa1 and used.fp2 is g0.fp2


def test_captured_step_dies_with_its_model(device):
    """A model keeps its captured step in `_graph`; the step must not keep the model alive in return, or the pair (captured graphs,
    their memory pools, the geometry's events) is freed by the cyclic collector at a moment of its choosing -- possibly inside
    another step's stream capture -- instead of when the model is dropped."""
    import gc
    import weakref
    from captra_amd.graph import TrackStepGraph
    from tests.test_model_gpu import _trainer
    trainer, cfg, sd, data = _trainer("bottle", device)
    model = trainer.model.eval()
    model.track_cfg["gt_label"] = False
    model.set_data(data)
    pose0 = {k: v.clone() for k, v in model.feed_dict[0]["gt_part"].items()}
    model._graph = TrackStepGraph(model, model.feed_dict[1]["points"], model.feed_dict[1]["points_mean"], pose0)
    assert model._graph.model is model
    torch.cuda.synchronize()
    step, net = weakref.ref(model._graph), weakref.ref(model)
    gc.collect()
    gc.disable()
    try:
        del trainer, model
        assert net() is None and step() is None
    finally:
        gc.enable()


def test_level1_stream_kernel_carries_both_backbones(device):
    """bf16 mode: both backbones' first level inside the sampler's launch (`stream_level1`), level 2's sampling with it."""
    from captra_amd import fused
    coord, rot = _net(True, device), _net(False, device, seed=9)
    cn, n3 = _cloud(device)
    with fused.use_mlp_dtype("bf16"):
        want_c, g0 = _run(coord, cn, n3)
        want_r, _ = _run(rot, cn, n3)
        for side in (None, torch.cuda.Stream()):
            with torch.no_grad():
                geom = coord.precompute_geometry(n3, side=side, stream_level1=(cn, None, [(rot, None), (coord, cn)]))
            torch.cuda.synchronize()
            assert geom.stream_scratch is not None and geom.level2_picks is not None, "the level-1 stream kernel did not run"
            assert set(geom.sa1.pooled) == {coord.sa1, rot.sa1}
            assert not fused.sa1_stream_gave_up(geom.stream_scratch)
            _assert_same_geometry(geom, g0, f"stream kernel, side={side is not None}")
            assert torch.equal(_run(coord, cn, n3, geom)[0], want_c)
            assert torch.equal(_run(rot, cn, n3, geom)[0], want_r)
            # level 1: 2 layouts + 3 lists + 2 pooled; level 2: 2 layouts + 2 lists; 2 weight pairs; level 2's picks (its coordinates ARE
            # level 2's layouts: once); the scratch buffer
            assert len(list(geom.tensors())) == len({id(t) for t in geom.tensors()}) == 7 + 4 + 4 + 1 + 1
