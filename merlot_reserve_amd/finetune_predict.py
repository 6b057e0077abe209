"""Predictions of a finetuned checkpoint: the counterpart of finetune/vcr/submit_to_leaderboard.py and finetune/tvqa/submit_to_leaderboard.py.

    python -m merlot_reserve_amd.finetune_predict {vcr,tvqa} CONFIG.yaml CKPT -fns PATTERN -num_files K -out FILE
        [-test_fns PATTERN -num_test_files K] [-output_grid_h H] [-output_grid_w W] [-val_batch_size N] [--split val|test]
        [--model-size Base|Large] [--seed S]

The forward-only model (MerlotReserveVCR / MerlotReserveTVQA.from_config(config, train=False): no optimizer state, no gradient buffer, no
backward buffers) is loaded from the checkpoint's `params` alone and run over PATTERN.format(0..K-1) in file order.  FILE gets one JSON line per
example (id, preds, logprobs, labels: finetune_eval.write_predictions); beside it the submission: <FILE stem>_submission.csv for VCR,
the folder <FILE stem>_submission/ (text, audio, joint) for TVQA.  There the examples of -fns go under --split (val by default); with
-test_fns a second pass fills the test split as well (its rows follow the first pass's in FILE), as the reference's script runs both.  A split
that was not run gets no prediction file.  meta.json names the model size of --model-size; without it the size is read from the config file's
NAME (not its directory): 'base' in it gives Base, anything else Large, the reference's rule."""
import argparse
import os
import sys


def build_parser():
    ap = argparse.ArgumentParser(description='MERLOT Reserve finetuned-model predictions (VCR, TVQA) on MI355X')
    ap.add_argument('task', choices=['tvqa', 'vcr'])
    ap.add_argument('pretrain_config_file')
    ap.add_argument('ckpt', help='a checkpoint file, or a directory of ckpt_<step> files (the latest)')
    ap.add_argument('-fns', required=True, help="shard pattern, e.g. 'val{:03d}of008.tfrecord'")
    ap.add_argument('-num_files', type=int, required=True)
    ap.add_argument('-out', required=True)
    ap.add_argument('-output_grid_h', type=int, default=12)
    ap.add_argument('-output_grid_w', type=int, default=20)
    ap.add_argument('-val_batch_size', type=int, default=32)
    ap.add_argument('--split', default='val', choices=['val', 'test'], help='TVQA: the split the examples of -fns belong to')
    ap.add_argument('-test_fns', default='', help='TVQA: shards of the test split, predicted in a second pass')
    ap.add_argument('-num_test_files', type=int, default=0)
    ap.add_argument('--model-size', default=None, choices=['Base', 'Large'], help="TVQA meta.json (default: from the config file's name)")
    ap.add_argument('--seed', type=int, default=0)
    return ap


def predict_config(config, task, args):
    """The task's configuration (finetune_train.task_overrides; the optimizer keys are not read) over the given shards."""
    from .finetune_train import task_overrides
    ns = argparse.Namespace(lr=0.0, ne=1, gpus=1, records_per_gpu=args.val_batch_size, train_size=args.val_batch_size,
                            output_grid_h=args.output_grid_h, output_grid_w=args.output_grid_w)
    config = task_overrides(config, task, ns)
    config['data'].update(val_fns=args.fns, num_val_files=int(args.num_files))
    return config


def model_size(args):
    if args.model_size:
        return args.model_size
    return 'Base' if 'base' in os.path.basename(args.pretrain_config_file).lower() else 'Large'


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.test_fns and (args.task != 'tvqa' or args.split != 'val' or args.num_test_files < 1):
        raise SystemExit('-test_fns is for TVQA, beside -fns as the val split, and needs -num_test_files')
    import torch
    from . import finetune_eval as E
    from . import finetune_records as FR
    from .checkpoint import load_checkpoint
    from .config import load_config
    from .finetune_train import model_and_batch

    task = args.task
    config = predict_config(load_config(args.pretrain_config_file), task, args)
    dev = torch.device('cuda', 0)
    model, dummy = model_and_batch(task, config, args.val_batch_size, dev, seed=args.seed, train=False)
    model.init_from_dummy_batch(dummy)
    model._load({'params': load_checkpoint(args.ckpt)['params']})
    def run(cfg):
        it = FR.finetune_val_input_fn_builder(cfg, task, workers=8, processes=False, sep_tokens=FR.SEP_TOKEN_IDS)
        return E.val_epoch(model, it, task)
    acc, rows = run(config)
    by_split = {args.split: rows}
    if args.test_fns:
        test_config = dict(config, data=dict(config['data'], val_fns=args.test_fns, num_val_files=int(args.num_test_files)))
        by_split['test'] = run(test_config)[1]
        rows = rows + by_split['test']
    E.write_predictions(rows, args.out)
    stem = os.path.splitext(args.out)[0]
    if task == 'vcr':
        sub = E.write_vcr_submission(rows, stem + '_submission.csv')
    else:
        sub = stem + '_submission'
        E.write_tvqa_submission(by_split, sub, model_size=model_size(args))
    print(f'{len(rows)} examples; accuracy of the first pass against the stored labels {acc}; predictions in {args.out}, submission in {sub}', flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
