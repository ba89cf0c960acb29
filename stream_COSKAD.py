#!/usr/bin/env python
"""stream_COSKAD.py -- the evaluation of eval_COSKAD.py as a stream: load <exp_dir>/<dataset>/<dir_name>/<load_ckpt> (and the pickled
scaler beside it), replay the test split's trajectories clip by clip, frame by frame, through coskad_amd.stream.StreamScorer -- all
persons of a clip interleaved by frame id, every track closed at the end of its clip -- then smooth the streamed clip vectors and take
the AUC with the host functions eval_COSKAD.py's scoring uses.  Prints the same `final AUC score:` line; --out DIR keeps the
pre-smoothing scores per clip as <scene>_<clip>.npy [num_transform, frames]."""
import argparse
import os
import pickle
from collections import OrderedDict

import numpy as np
import torch
import yaml
from sklearn.metrics import roc_auc_score

from coskad_amd.lit import LitEncoder, load_checkpoint
from coskad_amd.stream import StreamScorer
from coskad_amd.utils.argparser import init_sub_args
from coskad_amd.utils.eval_utils import eval_loss_type, score_process


def synthetic_trajectories(data, T):
    """The trajectories behind coskad_amd.utils.synthetic.make_dataset's window table: {(scene, clip, person): (frame ids from 1,
    rows [n, 34] = x1, y1, ...)} -- row f of a person is position 0 of its window f, the last window gives the last T rows."""
    x, trans, meta, _ = data
    keep = np.flatnonzero(trans.numpy() == 0)
    x, meta = x.numpy()[keep], meta.numpy()[keep]
    out = OrderedDict()
    for key in sorted({tuple(int(v) for v in r[:3]) for r in meta}):
        rows = np.flatnonzero((meta[:, :3] == key).all(1))
        rows = rows[np.argsort(meta[rows, 3], kind="stable")]
        w = x[rows]                                                    # [n - T + 1, 2, T, V], window s starts at row s
        traj = np.concatenate([w[:, :, 0], np.transpose(w[-1, :, 1:], (1, 0, 2))], 0)      # [n, 2, V]
        out[key] = (np.arange(1, traj.shape[0] + 1), np.ascontiguousarray(np.transpose(traj, (0, 2, 1))).reshape(traj.shape[0], -1))
    return out


def replay_clip(scorer, trajs, tids):
    """one clip through the scorer, its persons interleaved by frame id; every track is closed at the end"""
    pos = {t: {int(f): i for i, f in enumerate(trajs[t][0])} for t in tids}
    for f in sorted({f for t in tids for f in pos[t]}):
        here = [t for t in tids if f in pos[t]]
        scorer.push(f, here, np.stack([trajs[t][1][pos[t][f]] for t in here]))
    scorer.close()


def main():
    parser = argparse.ArgumentParser(description='Pose_AD_Experiment')
    parser.add_argument('-c', '--config', type=str, required=True)
    parser.add_argument('--out', type=str, default=None)        # <scene>_<clip>.npy: the streamed scores before smoothing
    cli = parser.parse_args()
    args = argparse.Namespace(**yaml.load(open(cli.config), Loader=yaml.FullLoader))
    args, dataset_args, ae_args, res_args, opt_args = init_sub_args(args)
    torch.cuda.set_device(0)
    if int(getattr(args, 'pad_size', -1)) != -1:
        raise ValueError("stream_COSKAD.py: absence padding (pad_size) needs a person's whole row and is not streamed; set pad_size: -1")
    if args.use_decoder:                             # wrapper selection order: eval_COSKAD.py:55-83
        from coskad_amd.lit import LitAutoEncoder
        model = LitAutoEncoder(args).cuda()
        model.rec_loss_weight = getattr(args, 'eval_rec_loss_weight', 0)
        model.score_type = eval_loss_type(model.rec_loss_weight)
    elif args.use_vae:
        from coskad_amd.lit import LitVAE
        model = LitVAE(args).cuda()                  # StreamScorer refuses it and says why
    else:
        model = LitEncoder(args).cuda()
    path = os.path.join(args.exp_dir, args.dataset_choice, args.dir_name, args.load_ckpt)
    print('Loading model from {}'.format(path))
    load_checkpoint(model, path)
    model.model.eval()
    K = max(1, int(args.dataset_num_transform))
    T = args.dataset_seg_len
    if args.data_dir == 'synthetic':
        from coskad_amd.utils.synthetic import make_dataset
        test, gts = make_dataset(n_scenes=2, n_clips=3, n_persons=3, clip_len=200, num_transform=K, anomaly=True, seed=args.seed + 1, T=T)
        trajs = synthetic_trajectories(test, T)
        # the generator's rows are normalised already; its transformation 1 swaps x and y
        mats = np.stack([np.eye(3, dtype=np.float32), np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)])
        if K > 2:
            raise ValueError("stream_COSKAD.py: the synthetic generator has two transformations")
        scorer = StreamScorer(model, None, None, max_tracks=16, num_transform=K, clip_frames=1, mats=mats[:K])
        hr_masks = None
    else:
        # eval_COSKAD.py:107-116: test split of the Morais-format tree, scaler pickled by the training run
        from coskad_amd.utils.dataset import load_trajectories
        root = getattr(dataset_args, 'path_to_robust', getattr(args, 'data_dir', ''))
        sub = 'testing' if 'test' in args.split else ('training' if 'train' in args.split else 'validating')
        trajs = OrderedDict()
        for tid, v in load_trajectories(os.path.join(root, sub, 'trajectories'), split=args.split).items():
            scene, clip = (int(s) for s in tid.split('_')[0].split('-'))
            trajs[(scene, clip, int(tid.split('_')[1]))] = v
        scaler = None
        if getattr(dataset_args, 'normalize_pose', True):
            with open(os.path.join(os.path.dirname(path), 'local_robust.pickle'), 'rb') as f:
                scaler = pickle.load(f)
        gts = model._load_gts()
        hr_masks = model._load_hr_masks()
        live = max(len([t for t in trajs if t[:2] == c]) for c in {t[:2] for t in trajs})
        scorer = StreamScorer(model, scaler, getattr(dataset_args, 'vid_res', [1080, 720]), max_tracks=max(live, 1), num_transform=K,
                              clip_frames=1)
    raw = {}
    for key in sorted(gts):
        n = int(np.asarray(gts[key]).shape[0])
        scorer.reset(clip_frames=n)
        tids = [t for t in trajs if t[:2] == key]
        if tids:
            replay_clip(scorer, trajs, tids)
        raw[key] = scorer.clip_scores().cpu().numpy()            # a clip without detections scores 0 everywhere
    if cli.out:
        os.makedirs(cli.out, exist_ok=True)
        for (sc, cl), v in raw.items():
            np.save(os.path.join(cli.out, f"{sc}_{cl}.npy"), v)
    hr_masks = hr_masks or {}
    keys = sorted(gts)
    per_t = [np.concatenate([score_process(raw[k][t][hr_masks[k]] if k in hr_masks else raw[k][t], win_size=int(getattr(args, 'smoothing', 50)),
                                           dataname=args.dataset_choice, use_scaler=False) for k in keys]) for t in range(K)]
    gt = np.concatenate([np.asarray(gts[k])[hr_masks[k]] if k in hr_masks else np.asarray(gts[k]) for k in keys])
    auc = roc_auc_score(gt, np.mean(np.stack(per_t, 0), 0))
    print('final AUC score: {}'.format(auc))


if __name__ == '__main__':
    main()
