#!/usr/bin/env python
"""Drop-in for the reference's ``train.py`` (:21-76): same flags (-o/--opt, -t/--train_set, -t1/--test_set, -r/--resume, --gpu_id), same
yml schema, same checkpoint files and metric lines.  What trains is the head (``VQAHead``, or ``simpleVQAHead`` for model key
``simpleVQA``) on features of the frozen trunk (``Trainer.finetune_head``): ``optimizer.backbone_lr_mult`` must be 0.

    python train.py -o config/kwai_swin_grpb_synthetic_finetune.yml -r ./checkpoint/ --gpu_id 0
    python train.py -o config/kwai_simpleVQA_synthetic_finetune.yml -r ./checkpoint/ --gpu_id 0

With the yml key ``feature_bank: {draws, dtype}`` every train video is sampled ``draws`` times in the train phase and cached in a 16-bit
feature bank (``config/kwai_swin_grpb_synthetic_bank_finetune.yml``, ``config/kwai_simpleVQA_synthetic_bank_finetune.yml``).
"""
import argparse
import os
import sys

import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("-o", "--opt", type=str, default="config/kwai_swin_grpb_synthetic_finetune.yml", help="the option file")
    parser.add_argument("-t", "--train_set", type=str, default="train", help="target_set")
    parser.add_argument("-t1", "--test_set", type=str, default="val-ltest", help="target_set")
    parser.add_argument("-r", "--resume", type=str, default="./checkpoint/", help="where the checkpoints go")
    parser.add_argument("--gpu_id", type=str, default="0")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.opt, "r") as f:
        opt = yaml.safe_load(f)
    print(opt)
    os.makedirs(args.resume, exist_ok=True)
    import kvq_amd  # noqa: F401
    from kvq_amd.trainer import Trainer
    trainer = Trainer(args, opt)
    bests_n, bests = trainer.finetune_head()
    for tag, b in (("s", bests), ("n", bests_n)):
        print(f"""
                the best validation accuracy of the model-{tag} is as follows:
                SROCC: {b[0]:.4f}
                PLCC:  {b[1]:.4f}
                KROCC: {b[2]:.4f}
                RMSE:  {b[3]:.4f}.""")


if __name__ == "__main__":
    main()
