"""Helpers of the stream tests: the golden Morais CSV tree rebuilt from tests/golden/data_pipeline.npz (as tests/test_frame_table_host.py
does), its raw trajectories grouped into clips, and the replay of a clip frame by frame -- all persons of a clip interleaved by frame id."""
import os
from collections import OrderedDict

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden", "data_pipeline.npz")
BASE = dict(num_transform=5, seg_len=12, vid_res=[1080, 720], num_coords=2)


def build_tree(root, exp):
    """-> (root, exp) as strings: the CSV tree under `root`, the train split's scaler pickled under `exp`"""
    from coskad_amd.utils.dataset import PoseDatasetRobust
    g = np.load(GOLD)
    for k in g.files:
        if not k.startswith("csv."):
            continue
        _, split, folder, person = k.split(".")
        d = root / ("training" if split == "train" else "testing") / "trajectories" / folder
        d.mkdir(parents=True, exist_ok=True)
        np.savetxt(d / f"{person}.csv", g[k], delimiter=",", fmt="%.6f")
    PoseDatasetRobust(str(root), split="train", exp_dir=str(exp), seg_stride=2, **BASE)     # pickles the scaler the test split loads
    return str(root), str(exp)


def raw_trajectories(root, split="test"):
    """{(scene, clip, person): (frame ids int32 [n], raw pixel rows f32 [n, 34])} in the dataset's trajectory order"""
    from coskad_amd.utils.dataset import load_trajectories
    sub = "training" if split == "train" else "testing"
    out = OrderedDict()
    for tid, (frames, coords) in load_trajectories(os.path.join(root, sub, "trajectories")).items():
        scene, clip = (int(v) for v in tid.split("_")[0].split("-"))
        out[(scene, clip, int(tid.split("_")[1]))] = (frames, coords)
    return out


def clips_of(trajs):
    """{(scene, clip): [track ids]} in sorted clip order"""
    out = OrderedDict()
    for tid in trajs:
        out.setdefault(tid[:2], []).append(tid)
    return OrderedDict(sorted(out.items()))


def frame_events(trajs, tids):
    """The clip's frames in ascending frame id: [(frame id, [track ids present], rows [n, 34])]"""
    ids = sorted({int(f) for t in tids for f in trajs[t][0]})
    pos = {t: {int(f): i for i, f in enumerate(trajs[t][0])} for t in tids}
    out = []
    for f in ids:
        here = [t for t in tids if f in pos[t]]
        out.append((f, here, np.stack([trajs[t][1][pos[t][f]] for t in here])))
    return out
