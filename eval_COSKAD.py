#!/usr/bin/env python
"""eval_COSKAD.py -- reference CLI (eval_COSKAD.py:46-253): load <exp_dir>/<dataset>/<dir_name>/<load_ckpt>,
predict latents on the test split, score windows -> frames -> clips, print the AUC."""
import argparse
import os

import torch
import yaml

from coskad_amd import parallel
from coskad_amd.lit import LitEncoder, Trainer
from coskad_amd.utils.argparser import init_sub_args
from coskad_amd.utils.synthetic import batches, make_dataset


def main():
    parser = argparse.ArgumentParser(description='Pose_AD_Experiment')
    parser.add_argument('-c', '--config', type=str, required=True)
    # the reference's per-clip / per-transformation log (eval_COSKAD.py:222-242); the yaml key `eval_report: true` asks for the same
    parser.add_argument('--report', action='store_true')
    parser.add_argument('--report-dir', type=str, default=None)      # report.json + <scene>_<clip>.npy (implies --report)
    # per clip <scene>_<clip>_attribution.npy [persons, frames, V] (gradient x input of the window scores, mean over the covering windows
    # and the transformations, NaN where a person is absent) and <scene>_<clip>_persons.npy; one-class encoders only
    parser.add_argument('--attribution-dir', type=str, default=None)
    # per clip <scene>_<clip>_error_map.npy [persons, frames, V] (the per-joint reconstruction error of the windows, mean over the covering
    # windows and the transformations, NaN where a person is absent) and <scene>_<clip>_persons.npy; autoencoder / VAE configs whose
    # score has a reconstruction term
    parser.add_argument('--error-map-dir', type=str, default=None)
    cli = parser.parse_args()
    args = argparse.Namespace(**yaml.load(open(cli.config), Loader=yaml.FullLoader))
    if cli.report or cli.report_dir:
        args.eval_report = True
    args, dataset_args, ae_args, res_args, opt_args = init_sub_args(args)
    torch.cuda.set_device(0)
    if args.use_decoder:                             # wrapper selection order: eval_COSKAD.py:55-83
        from coskad_amd.lit import LitAutoEncoder
        model = LitAutoEncoder(args).cuda()
        from coskad_amd.utils.eval_utils import eval_loss_type
        # eval_COSKAD.py:58-66: the script's constant, 0, selects 'hyp'.  `eval_rec_loss_weight` (no key of the reference's yamls; 0
        # unless set) stands for that constant: > 100 selects 'rec', any other non-zero value 'rec+hyp'
        model.rec_loss_weight = getattr(args, 'eval_rec_loss_weight', 0)
        model.score_type = eval_loss_type(model.rec_loss_weight)
    elif args.use_vae:
        from coskad_amd.lit import LitVAE
        model = LitVAE(args).cuda()
    else:
        model = LitEncoder(args).cuda()
    path = os.path.join(args.exp_dir, args.dataset_choice, args.dir_name, args.load_ckpt)
    print('Loading model from {}'.format(path))
    trainer = Trainer()
    if args.data_dir == 'synthetic':
        test, gts = make_dataset(n_scenes=2, n_clips=3, n_persons=3, clip_len=200, num_transform=args.dataset_num_transform,
                                 anomaly=True, seed=args.seed + 1, T=args.dataset_seg_len)
        model.gts = gts
        loader_fn = lambda: batches(test, args.dataset_batch_size)
        out = trainer.predict(model, loader_fn, ckpt_path=path)
    else:
        # eval_COSKAD.py:107-116: test split of the Morais-format tree, scaler pickled by the training run
        from coskad_amd.utils.dataset import get_dataset_and_loader
        dataset_args.exp_dir = os.path.dirname(path)
        _, loader = get_dataset_and_loader(dataset_args, split=args.split)
        loader_fn = lambda: loader
        out = trainer.predict(model, loader_fn, ckpt_path=path)
    auc = model.validation_epoch_end(out)
    report = getattr(model, 'last_report', None)
    if report is not None and parallel.rank() == 0:
        for line in list(report.lines())[:-1]:      # its last line is the one below
            print(line)
        if cli.report_dir:
            report.save(cli.report_dir)
    print('final AUC score: {}'.format(auc))
    if cli.attribution_dir and parallel.rank() == 0:
        from coskad_amd.attribution import dataset_attribution
        dataset_attribution(model, loader_fn, out, cli.attribution_dir)
        print('attribution maps written to {}'.format(cli.attribution_dir))
    if cli.error_map_dir and parallel.rank() == 0:
        from coskad_amd.attribution import dataset_error_maps
        dataset_error_maps(model, loader_fn, out, cli.error_map_dir)
        print('error maps written to {}'.format(cli.error_map_dir))


if __name__ == '__main__':
    main()
