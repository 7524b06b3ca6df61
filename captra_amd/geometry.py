"""What a PointNet++ MSG backbone derives from a cloud's coordinates alone, as the object that is handed around.

`PointNet2Msg.precompute_geometry*` build a `CloudGeometry`, `PointNet2Msg.forward(geom=...)` and the SA modules consume it and
fill in what is missing, and two backbones on the same cloud (CoordinateNet / RotationNet of one part) share one.  Records
only: nothing here launches anything.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from itertools import chain

import torch


@dataclass(slots=True, eq=False)
class LevelGeometry:
    """One set-abstraction level."""
    new_xyz_n3: torch.Tensor | None = None          # (B,M,3) the sampled centres ...
    new_xyz: torch.Tensor | None = None             # ... and (B,3,M); None = not sampled yet
    idx_list: list | None = None                    # [(B,M,K) int32] per scale; None until the ball query ran
    pooled: dict = field(default_factory=dict)      # SA module -> its finished (B,C,M) features (the level-1 stream kernel ran it)
    windows: list | None = None                     # the streamed sampler's [(first centre, count, event)]


@dataclass(slots=True, eq=False)
class CloudGeometry:
    sa1: LevelGeometry = field(default_factory=LevelGeometry)
    sa2: LevelGeometry | None = None                # None: level 1 only
    fp1: tuple | None = None                        # (idx, weight) of fused.three_nn_weights: the cloud among level 1's centres
    fp2: tuple | None = None                        # ... level 1's centres among level 2's
    level2_picks: tuple | None = None               # (idx, (B,M2,3), (B,3,M2)): the level-1 stream kernel sampled level 2 too
    stream_scratch: torch.Tensor | None = None      # the level-1 stream kernel's scratch buffer (holds its give-up word)
    ready: object | None = None                     # event behind the streamed form's last launch (level 2 waits for it)
    keep: tuple = ()                                # tensors that only have to stay alive with the geometry

    def tensors(self):
        """Every device tensor of the geometry, once."""
        levels = [lv for lv in (self.sa1, self.sa2) if lv is not None]
        groups = [(lv.new_xyz_n3, lv.new_xyz, *(lv.idx_list or ()), *lv.pooled.values()) for lv in levels]
        groups += [self.fp1 or (), self.fp2 or (), self.level2_picks or (), (self.stream_scratch,), self.keep]
        seen = set()
        for t in chain(*groups):
            if torch.is_tensor(t) and id(t) not in seen:
                seen.add(id(t))
                yield t

    def record_stream(self, *streams):
        for t in self.tensors():
            for st in streams:
                t.record_stream(st)
