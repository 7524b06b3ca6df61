"""fused.pointwise_mlp2 on two sources the allocator put further apart than one buffer descriptor spans: where two small tensors land
is no property of the call, so the wrapper copies them into one buffer and launches as ever -- the same bits as for neighbours."""
import numpy as np
import pytest


@pytest.mark.gpu
@pytest.mark.parametrize("c,c2,cout,L,bcast", [(3, 70, 96, 75, False), (64, 128, 128, 130, True)])
def test_far_apart_sources_give_the_neighbours_bits(device, monkeypatch, c, c2, cout, L, bcast):
    import torch
    from captra_amd import fused
    rng = np.random.default_rng(c + c2 + cout + L)
    dev = lambda a: torch.from_numpy(a).to(device)          # noqa: E731
    x = dev(rng.standard_normal((3, c, L)).astype(np.float32))
    x2 = dev(rng.standard_normal((3, c2, 1 if bcast else L)).astype(np.float32))
    lin = fused.pack(dev((rng.standard_normal((c + c2, cout)) / np.sqrt(c + c2)).astype(np.float32)), dev(rng.standard_normal(cout).astype(np.float32)))
    near = fused.pointwise_mlp2(x, x2, lin, 1)
    assert near is not None
    monkeypatch.setattr(fused, "MLP2_SPAN_LIMIT", 0)         # every pair counts as too far apart
    far = fused.pointwise_mlp2(x, x2, lin, 1)
    assert far is not None and torch.equal(far.view(torch.int32), near.view(torch.int32))
