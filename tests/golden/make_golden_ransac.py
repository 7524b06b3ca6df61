"""Golden fixture G17: the reference's RANSAC pose fit (datasets/nocs_data/preproc_nocs/align_pose.py::pose_fit) on seeded clouds.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ransac.py [--ref /root/reference]

Nothing of the reference is copied: align_pose is imported read-only from --ref and run in float64 on the float32 clouds of
tests/ransac_judge.py's recipe.  Run-time adjustment (monkey patch, not an edit): its `random_choice_noreplace` is wrapped so that
the triples it draws are recorded -- the fit is a function of them.  Written: per case the inputs (src, tgt (K,3) fp32, th), the
recorded triples (64,3), the reference's rotation / scale / translation, and `none` = 1 where pose_fit returned None (a cloud of
gross outliers only: fewer than three inliers; its pose arrays are zeros).  Data only, ~60 KB.
"""
import argparse
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))

from tests import ransac_judge as J  # noqa: E402

CASES = ((0, 3), (1, 5), (2, 40), (3, 257), (4, 400), (5, 300))       # (seed, members); the last one is the None case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=str(HERE / "g17_pose_fit_ransac.npz"))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.ref) / "datasets" / "nocs_data" / "preproc_nocs"))
    import align_pose as AP

    drawn = []
    inner = AP.random_choice_noreplace

    def recording(idx_range, n_sample, num_draw):
        out = inner(idx_range, n_sample, num_draw)
        drawn.append(np.array(out))
        return out
    AP.random_choice_noreplace = recording

    blob = {"num_cases": np.int64(len(CASES))}
    for k, (seed, count) in enumerate(CASES):
        rng = np.random.default_rng(1700 + seed)
        S, T, th, true_in, _ = J.recipe_cloud(rng, count)
        want_none = k == len(CASES) - 1
        if want_none:       # every target a gross outlier: no hypothesis gathers three inliers
            T = (np.array([0.1, -0.2, 2.0]) + (rng.random((count, 3)) - 0.5) * 100 * th).astype(np.float32)
        np.random.seed(1700 + k)
        model = AP.pose_fit(S.astype(np.float64), T.astype(np.float64), num_hyps=64, inlier_th=th)
        triples = drawn[-1]
        assert triples.shape == (64, 3)
        assert (model is None) == want_none, (k, model)
        blob[f"src{k}"], blob[f"tgt{k}"], blob[f"th{k}"], blob[f"triples{k}"] = S, T, np.float64(th), triples.astype(np.int32)
        blob[f"none{k}"] = np.int64(model is None)
        blob[f"rot{k}"] = np.zeros((3, 3)) if model is None else np.asarray(model["rotation"], np.float64).reshape(3, 3)
        blob[f"scale{k}"] = np.float64(0) if model is None else np.float64(np.asarray(model["scale"]).reshape(()))
        blob[f"trans{k}"] = np.zeros(3) if model is None else np.asarray(model["translation"], np.float64).reshape(3)
    np.savez_compressed(args.out, **blob)
    print("wrote", args.out, Path(args.out).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
