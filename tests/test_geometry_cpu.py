"""The shared cloud geometry's record types (captra_amd/geometry.py) and what PointNet2Msg does with them off the GPU.  No GPU.

The operator layer has no CPU path (captra_amd/pointnet_utils.py: every function runs the HIP operator and raises on CPU tensors),
so a whole backbone forward on the CPU raises, before this object as after it.  The layer-by-layer path that training runs is
exercised here all the same, with plain-torch stand-ins for the five operators it calls; its output is pinned by
tests/golden/geometry_cpu_forward.npz, which the same stand-ins produced with the dict-based geometry this object replaced."""
from pathlib import Path

import numpy as np
import pytest
import torch

from captra_amd.geometry import CloudGeometry, LevelGeometry

GOLDEN = Path(__file__).parent / "golden" / "geometry_cpu_forward.npz"


def _t():
    return torch.zeros(1)


def test_tensors_yields_every_tensor_once():
    module_a, module_b, event = object(), object(), object()
    sa1 = LevelGeometry(_t(), _t(), [_t(), _t(), _t()], {module_a: _t(), module_b: _t()}, windows=[(0, 8, event), (8, 8, event)])
    sa2 = LevelGeometry(_t(), _t(), [_t(), _t()])
    geom = CloudGeometry(sa1=sa1, sa2=sa2, fp1=(_t(), _t()), fp2=(_t(), _t()), level2_picks=(_t(), sa2.new_xyz_n3, sa2.new_xyz),
                         stream_scratch=_t(), ready=event, keep=(_t(), sa1.idx_list[0]))
    want = [sa1.new_xyz_n3, sa1.new_xyz, *sa1.idx_list, *sa1.pooled.values(), sa2.new_xyz_n3, sa2.new_xyz, *sa2.idx_list, *geom.fp1, *geom.fp2,
            geom.level2_picks[0], geom.stream_scratch, geom.keep[0]]
    got = list(geom.tensors())
    assert len(got) == len(want) == 7 + 4 + 4 + 3
    assert all(g is w for g, w in zip(got, want))           # each once (a tensor two fields share included), nothing else


def test_level1_only_geometry_yields_level1_only():
    sa1 = LevelGeometry(_t(), _t(), [_t(), _t(), _t()])
    got = list(CloudGeometry(sa1=sa1).tensors())
    assert all(g is w for g, w in zip(got, [sa1.new_xyz_n3, sa1.new_xyz, *sa1.idx_list])) and len(got) == 5
    assert list(CloudGeometry().tensors()) == []
    assert len(list(CloudGeometry(sa1=LevelGeometry(_t(), _t())).tensors())) == 2               # lists not made yet: the sampling alone


def test_fields_are_fixed():
    """A misspelt field is an error, not a silent None."""
    with pytest.raises(AttributeError):
        CloudGeometry().fp3 = None
    with pytest.raises(AttributeError):
        LevelGeometry().chunks = []
    with pytest.raises(TypeError):
        CloudGeometry(scratch=None)


def _backbone(use_xyz=True):
    from captra_amd.backbones import PointNet2Msg
    from captra_amd.configs import make_config
    from captra_amd.synthetic import make_state_dict
    cfg = make_config("1")
    cfg["device"] = "cpu"
    net = PointNet2Msg(cfg, 128, use_xyz_feat=use_xyz)
    net.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=4))
    return net


def _cloud(n=1024):
    return torch.from_numpy((np.random.default_rng(11).random((1, 3, n), dtype=np.float32) - 0.5) * 0.8)


def test_precompute_geometry_is_none_off_the_fused_path():
    net, cn = _backbone(), _cloud()
    n3 = cn.transpose(1, 2).contiguous()
    assert net.eval().precompute_geometry(n3) is None                                   # a CPU cloud
    assert net.precompute_geometry_streamed(n3, 4, None) is None
    net.train()
    assert net.precompute_geometry(n3) is None and net.precompute_geometry(n3, level1_only=True) is None      # training mode
    assert net.precompute_geometry_streamed(n3, 4, None) is None


def test_cpu_forward_raises_as_before():
    from captra_amd._lib import CaptraHipError
    with pytest.raises(CaptraHipError), torch.no_grad():
        _backbone().eval()(_cloud(256))


# ---- plain-torch stand-ins for the operators of the layer-by-layer path (same signatures as captra_amd.pointnet_lib.pointnet2_utils)
def _d2(a, b):
    """(B,S,3), (B,N,3) -> (B,S,N) squared distances, one fixed order of operations."""
    d = a.unsqueeze(2) - b.unsqueeze(1)
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _fps(xyz, m):
    b, n, _ = xyz.shape
    idx, dist = torch.zeros(b, m, dtype=torch.int64), torch.full((b, n), 1e10)
    for j in range(1, m):
        dist = torch.minimum(dist, _d2(xyz[torch.arange(b), idx[:, j - 1]].unsqueeze(1), xyz)[:, 0])
        idx[:, j] = dist.argmax(1)
    return idx.int()


def _ball_query(radius, k, xyz, new_xyz):
    n = xyz.shape[1]
    order = torch.where(_d2(new_xyz, xyz) < radius * radius, torch.arange(n), torch.tensor(n)).sort(dim=2)[0][:, :, :k]
    return torch.where(order == n, order[:, :, :1], order).int()


def _group(feat, idx):
    b, c, _ = feat.shape
    return torch.gather(feat.unsqueeze(2).expand(-1, -1, idx.shape[1], -1), 3, idx.long().unsqueeze(1).expand(-1, c, -1, -1))


def _three_nn(unknown, known):
    d, idx = _d2(unknown, known).topk(3, dim=2, largest=False)
    return d.sqrt(), idx.int()


def _three_interpolate(points, idx, weight):
    return (_group(points, idx) * weight.unsqueeze(1)).sum(-1)


@pytest.fixture
def torch_ops(monkeypatch):
    from captra_amd.pointnet_lib import pointnet2_utils as futils
    for name, fn in (("furthest_point_sample", _fps), ("ball_query", _ball_query), ("grouping_operation", _group), ("three_nn", _three_nn),
                     ("three_interpolate", _three_interpolate)):
        monkeypatch.setattr(futils, name, fn)


def test_layer_by_layer_forward_without_geometry_is_unchanged(torch_ops):
    """The non-fused path (what training and a CPU tensor take) with geom=None: the output the dict-based code gave, and the
    geometry it sampled on the way left in `last_geom` (no lists, no weights: this path keeps none).  Tolerance: the output goes
    through 13 conv + BatchNorm layers of at most 1539 terms per sum in fp32, whose order of summation is the CPU's business; the
    bound is 1e-4 relative to the output's scale, a hundred times that path's rounding and far below any change of a pick."""
    net, cn = _backbone().eval(), _cloud()
    with torch.no_grad():
        out = net(cn)
    want = torch.from_numpy(np.load(GOLDEN)["out_stride16"])
    assert out.shape == (1, 128, 1024)
    assert float((out[0, :, ::16] - want).abs().max()) <= 1e-4 * float(want.abs().max())
    g = net.last_geom
    assert g.sa1.new_xyz.shape == (1, 3, 512) and g.sa2.new_xyz_n3.shape == (1, 128, 3)
    assert g.sa1.idx_list is None and g.fp1 is None and g.fp2 is None
    with torch.no_grad():
        again = net(cn, geom=g)                      # handed its own samplings back: the same output, the same level objects
    assert torch.equal(again, out) and net.last_geom.sa1 is g.sa1
