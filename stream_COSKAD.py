#!/usr/bin/env python
"""stream_COSKAD.py -- the evaluation of eval_COSKAD.py as a stream: load <exp_dir>/<dataset>/<dir_name>/<load_ckpt> (and the pickled
scaler beside it), replay the test split's trajectories clip by clip, frame by frame, through coskad_amd.stream.StreamScorer -- all
persons of a clip interleaved by frame id, every track closed at the end of its clip -- then smooth the streamed clip vectors and take
the AUC with the host functions eval_COSKAD.py's scoring uses.  Prints the same `final AUC score:` line; --out DIR keeps the
pre-smoothing scores per clip as <scene>_<clip>.npy [num_transform, frames].

--cameras N replays N clips at a time through one coskad_amd.stream.StreamBank: clip i of a group is camera i, the cameras' frames are
interleaved tick by tick (one bank push serves them all), and each clip ends with `finish`.  The printed line is the same.
--smoothed-out DIR additionally writes the scores the bank smoothed on the device at a lag of 120 frames, as
<scene>_<clip>_smoothed.npy [num_transform, frames] (implies --cameras 1 where --cameras is not given).
--attribution-dir DIR (one-class encoders) / --error-map-dir DIR (autoencoder) stream with `maps=True` and, after the AUC line, write
the files eval_COSKAD.py's options of those names write -- <scene>_<clip>_attribution.npy or <scene>_<clip>_error_map.npy [persons,
frames, V] and <scene>_<clip>_persons.npy -- from the per-frame maps the stream handed out; with and without --cameras."""
import argparse
import os
import pickle
from collections import OrderedDict

import numpy as np
import torch
import yaml
from sklearn.metrics import roc_auc_score

from coskad_amd.lit import LitEncoder, load_checkpoint
from coskad_amd.stream import StreamBank, StreamScorer
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


class MapSink:
    """The per-joint maps a replay hands out (`maps=True`), kept on the device until the replay is over: which (track, frame id) every
    column of every `frame_maps` belongs to, and the tracks that completed a window -- the persons of the offline scoring plan."""

    def __init__(self):
        self.final, self.parts, self.windowed = [], [], set()

    def keep(self, out, track=lambda t: t):
        """`track`: an output's track id -> (scene, clip, person)"""
        self.windowed.update(track(t) for t in out.tracks)
        if out.frame_maps is not None:
            self.final += [(track(t), f) for t, f in out.final]
            self.parts.append(out.frame_maps)

    def save(self, directory, keys, lengths, K, V, suffix):
        """eval_utils.save_attribution on a plan-shaped view of the stream: per transformation and clip the persons that had a window,
        a row per frame of the clip, NaN where the stream made no map -- so the files are the offline route's, formula and all."""
        from types import SimpleNamespace
        from coskad_amd.utils.eval_utils import save_attribution
        persons = [(k, c, t[2]) for k in range(K) for c, key in enumerate(keys) for t in sorted(self.windowed) if t[:2] == key]
        person_n = np.array([lengths[keys[c]] for _, c, _ in persons], dtype=np.int64)
        row_ptr = np.concatenate([[0], np.cumsum(person_n)]).astype(np.int64)
        start = {(k, *keys[c], p): int(row_ptr[i]) for i, (k, c, p) in enumerate(persons)}
        maps = np.full((int(row_ptr[-1]), V), np.nan, dtype=np.float64)
        got = torch.cat(self.parts, 1).cpu().numpy() if self.parts else np.zeros((K, 0, V))
        for q, (t, f) in enumerate(self.final):
            if t in self.windowed and 1 <= f <= lengths[t[:2]]:
                for k in range(K):
                    maps[start[(k, *t)] + f - 1] = got[k, q]
        plan = SimpleNamespace(row_ptr=torch.from_numpy(row_ptr), clip_keys=list(keys),
                               person_clip=np.array([c for _, c, _ in persons], dtype=np.int64), person_n=person_n,
                               person_keys=np.array([(k, *keys[c], p) for k, c, p in persons], dtype=np.int64).reshape(-1, 4))
        save_attribution(directory, maps, plan, suffix=suffix)


def replay_clip(scorer, trajs, tids, sink=None):
    """one clip through the scorer, its persons interleaved by frame id; every track is closed at the end"""
    pos = {t: {int(f): i for i, f in enumerate(trajs[t][0])} for t in tids}
    for f in sorted({f for t in tids for f in pos[t]}):
        here = [t for t in tids if f in pos[t]]
        out = scorer.push(f, here, np.stack([trajs[t][1][pos[t][f]] for t in here]))
        if sink is not None:
            sink.keep(out)
    out = scorer.close()
    if sink is not None:
        sink.keep(out)


def replay_group(bank, trajs, group, lengths, sink=None):
    """The clips `group` = [(scene, clip)] through the bank, clip i on camera i: every tick pushes the next frame of every camera that
    has one (frames 1 .. n of a clip, nobody in view included), a camera whose clip is over is finished.
    -> ({key: clip vector [K, n]}, {key: smoothed [K, n]} with `bank.smooth`), on the host"""
    frames, pos, tids = {}, {}, {}
    for cam, key in enumerate(group):
        bank.reset(cam, clip_frames=lengths[key])
        tids[cam] = [t for t in trajs if t[:2] == key]
        pos[cam] = {t: {int(f): i for i, f in enumerate(trajs[t][0])} for t in tids[cam]}
        frames[cam] = sorted(set(range(1, lengths[key] + 1)) | {f for t in tids[cam] for f in pos[cam][t]})
    pieces = {cam: [] for cam in frames}

    def keep(out):
        at = 0
        for cam, _, count in out.smoothed:
            pieces[cam].append(out.smoothed_scores[:, at:at + count])
            at += count
        if sink is not None:
            sink.keep(out, track=lambda t: t[1])        # the bank's tracks are (cam, track id)

    for tick in range(max(len(f) for f in frames.values())):
        batch = {}
        for cam, fr in frames.items():
            if tick < len(fr):
                here = [t for t in tids[cam] if fr[tick] in pos[cam][t]]
                batch[cam] = (fr[tick], here, np.stack([trajs[t][1][pos[cam][t][fr[tick]]] for t in here]) if here else np.zeros((0, 34)))
        keep(bank.push(batch))
        for cam, fr in frames.items():
            if tick == len(fr) - 1:
                keep(bank.finish(cam))
    raw = {key: bank.clip_scores(cam).cpu().numpy() for cam, key in enumerate(group)}
    smoothed = {key: torch.cat(pieces[cam], 1).cpu().numpy() for cam, key in enumerate(group)} if bank.smooth else {}
    return raw, smoothed


def main():
    parser = argparse.ArgumentParser(description='Pose_AD_Experiment')
    parser.add_argument('-c', '--config', type=str, required=True)
    parser.add_argument('--out', type=str, default=None)        # <scene>_<clip>.npy: the streamed scores before smoothing
    parser.add_argument('--cameras', type=int, default=None)    # N clips at a time through one StreamBank, clip i on camera i
    parser.add_argument('--smoothed-out', type=str, default=None)       # <scene>_<clip>_smoothed.npy: the bank's device-smoothed scores
    # eval_COSKAD.py's map files from the stream (maps=True): <scene>_<clip>_attribution.npy of a one-class encoder,
    # <scene>_<clip>_error_map.npy of the autoencoder, [persons, frames, V] float32, and <scene>_<clip>_persons.npy
    parser.add_argument('--attribution-dir', type=str, default=None)
    parser.add_argument('--error-map-dir', type=str, default=None)
    cli = parser.parse_args()
    if cli.attribution_dir and cli.error_map_dir:
        parser.error("--attribution-dir is the map of the one-class encoders, --error-map-dir the autoencoder's: one wrapper, one map")
    maps = bool(cli.attribution_dir or cli.error_map_dir)
    n_cams = cli.cameras if cli.cameras is not None else (1 if cli.smoothed_out else None)
    if n_cams is not None and n_cams < 1:
        parser.error("--cameras: at least 1")
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
    if cli.attribution_dir and (args.use_decoder or args.use_vae):
        model.window_attribution(None)               # the wrapper's own refusal: the map of a decoder model is --error-map-dir
    if cli.error_map_dir and not args.use_decoder:
        model.window_error_map(None)                 # likewise: a one-class encoder has --attribution-dir
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
        if n_cams is None:
            scorer = StreamScorer(model, None, None, max_tracks=16, num_transform=K, clip_frames=1, mats=mats[:K], maps=maps)
        else:
            scorer = StreamBank(model, None, {c: dict(vid_res=None, clip_frames=1) for c in range(n_cams)}, max_tracks=16 * n_cams,
                                num_transform=K, mats=mats[:K], smooth=bool(cli.smoothed_out), maps=maps)
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
        res = getattr(dataset_args, 'vid_res', [1080, 720])
        if n_cams is None:
            scorer = StreamScorer(model, scaler, res, max_tracks=max(live, 1), num_transform=K, clip_frames=1, maps=maps)
        else:
            scorer = StreamBank(model, scaler, {c: dict(vid_res=res, clip_frames=1) for c in range(n_cams)},
                                max_tracks=max(live, 1) * n_cams, num_transform=K, smooth=bool(cli.smoothed_out), maps=maps)
    raw, smoothed = {}, {}
    sink = MapSink() if maps else None
    keys = sorted(gts)
    lengths = {key: int(np.asarray(gts[key]).shape[0]) for key in keys}
    if n_cams is not None:
        for g in range(0, len(keys), n_cams):
            a, b = replay_group(scorer, trajs, keys[g:g + n_cams], lengths, sink)
            raw.update(a)
            smoothed.update(b)
    for key in keys if n_cams is None else []:
        scorer.reset(clip_frames=lengths[key])
        tids = [t for t in trajs if t[:2] == key]
        if tids:
            replay_clip(scorer, trajs, tids, sink)
        raw[key] = scorer.clip_scores().cpu().numpy()            # a clip without detections scores 0 everywhere
    if cli.out:
        os.makedirs(cli.out, exist_ok=True)
        for (sc, cl), v in raw.items():
            np.save(os.path.join(cli.out, f"{sc}_{cl}.npy"), v)
    if cli.smoothed_out:
        os.makedirs(cli.smoothed_out, exist_ok=True)
        for (sc, cl), v in smoothed.items():
            np.save(os.path.join(cli.smoothed_out, f"{sc}_{cl}_smoothed.npy"), v)
    hr_masks = hr_masks or {}
    per_t = [np.concatenate([score_process(raw[k][t][hr_masks[k]] if k in hr_masks else raw[k][t], win_size=int(getattr(args, 'smoothing', 50)),
                                           dataname=args.dataset_choice, use_scaler=False) for k in keys]) for t in range(K)]
    gt = np.concatenate([np.asarray(gts[k])[hr_masks[k]] if k in hr_masks else np.asarray(gts[k]) for k in keys])
    auc = roc_auc_score(gt, np.mean(np.stack(per_t, 0), 0))
    print('final AUC score: {}'.format(auc))
    if cli.attribution_dir:
        sink.save(cli.attribution_dir, keys, lengths, K, scorer.V, "attribution")
        print('attribution maps written to {}'.format(cli.attribution_dir))
    if cli.error_map_dir:
        sink.save(cli.error_map_dir, keys, lengths, K, scorer.V, "error_map")
        print('error maps written to {}'.format(cli.error_map_dir))


if __name__ == '__main__':
    main()
