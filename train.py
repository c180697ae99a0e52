#!/usr/bin/env python
"""Training entry point on the MI355X hot path (counterpart of the reference's train.py:10-34).

    python train.py --yaml=train --name=run
    python train.py --yaml=train --name=run --resume=true          # continue from outputs/run/models/latest.pth
    python train.py --yaml=train --name=scene --load=ckpt.pth --optim.lr_enc=0   # per-scene fine-tuning of the decoder

Options use the reference's ``--a.b.c=value`` grammar and YAML inheritance; the configured data sets are served by seeded
synthetic scenes when no dataset is on disk.  One GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def run(argv):
    import torch
    from matchnerf_amd import options
    from matchnerf_amd.coach import Coach

    opt = options.set(opt_cmd=options.parse_arguments(argv))
    options.save_options_file(opt)
    if not str(opt.device).startswith("cuda"):
        raise SystemExit("train.py: training needs a GPU (the forward and backward kernels have no CPU path)")
    with torch.cuda.device(opt.device):
        coach = Coach(opt)
        coach.build_networks()
        coach.load_dataset(splits=["train", "val", "test"])
        coach.setup_visualizer()
        coach.setup_optimizer()
        coach.restore_checkpoint()
        coach.train_model()
    return coach


if __name__ == "__main__":
    run(sys.argv[1:])
