"""Orchestration counterpart of the reference's Coach (coach.py:27-529): build the network from the registry, restore a
checkpoint per child, iterate batches, call the hot path, report PSNR - and, since ABI 10, the TRAINING loop (coach.py:87-300):
parameter groups / scheduler of the reference's recipe, ``train_iteration`` = zero_grad, HIP forward, L2 loss, HIP backward,
clip + AdamW (the loss is one launch and clip + step are three: optim.FusedAdamW; MNERF_FUSED_OPTIM=0: torch's ops), checkpoints in the reference's format, scalars to
``<output_path>/scalars.jsonl`` (TensorBoard only where it can be imported).  A dataset is anything that yields batches with the
reference's contract (images, extrinsics, intrinsics, near_fars[, depth, scene, view_ids]); ``synthetic`` is built in so the tools
run offline.

Data-parallel training (train.py starts one process per GPU of ``gpu_ids``): every rank holds a full replica and runs the iteration
above on its own ``batch_size`` scenes; between backward and clip + step the gradients of all ranks are summed and multiplied by fp32(1 / W)
(optim.GradBucket: two HIP launches around ONE collective; the torch optimizers take optim.reduce_gradients_torch), then every rank
clips and steps on identical values, so the replicas stay bit-identical with no later exchange.  The effective batch is W x
``batch_size`` and the learning rates are NOT rescaled.  Rank r draws its rays and offsets from ``seed + r`` (dist.reseed), the order
of the scenes comes from (seed, epoch) alone, rank 0's weights (and, on a resume, optimizer and scheduler state) are broadcast after
``restore_checkpoint``, and only rank 0 writes checkpoints, scalars and prints.  Validation and tests are sharded: batch bi of a
loader is rendered and scored by rank bi % W (on the device: csrc/metrics.hip), rank 0 assembles the one-process report.  ``gpu_ids`` longer than one WITHOUT a process
group of that size still raises in ``setup_optimizer``: the in-process DataParallel form is not built."""
import json
import math
import os
import time

import numpy as np
import torch

from . import checkpoint, datasets, metrics, synthetic
from . import dist as mdist
from .edict import EasyDict as edict
from .models import models_dict


def fused_optim_enabled():
    """``MNERF_FUSED_OPTIM`` (default 1): AdamW steps and the L2 loss of ``Coach`` run on csrc/optim.hip; 0 takes torch's
    expression, ``clip_grad_norm_`` and foreach AdamW (measured: DESIGN.md section 4, tools/train_tail_time.py)"""
    return os.environ.get("MNERF_FUSED_OPTIM", "1").lower() not in ("0", "off", "false", "no")


class SyntheticScenes:
    """Seeded stand-in for a dataset (no DTU/LLFF/Blender data offline)."""

    def __init__(self, name, cfg, n_src_views, shuffle=False, rank=0, world=1, seed=None):
        self.name = name
        self.shuffle = shuffle  # training: a fresh order of the scenes every epoch (torch's generator)
        # data-parallel training (``seed`` given): the order comes from a generator of its own seeded by seed + epoch - the same on
        # every rank whatever the global generators hold -, rank r takes elements r, r + world, ... and the tail that does not
        # divide is dropped, so every rank runs the same number of iterations (torch's DistributedSampler with drop_last)
        self.rank, self.world, self.seed, self.epoch = rank, world, seed, 0
        w, h = cfg.get("img_wh", [64, 64])
        self.kw = dict(height=h, width=w, n_src_views=n_src_views, wide=(name == "blender"),
                       near_far=(2.0, 6.0) if name == "blender" else (2.125, 4.525))
        n = cfg.get("max_len", -1)
        self.n = 2 if n in (None, -1) else n

    def get_name(self):
        return self.name

    def __len__(self):
        return self.n // self.world

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        if self.seed is None:
            return torch.randperm(self.n).tolist() if self.shuffle else list(range(self.n))
        order = list(range(self.n))
        if self.shuffle:
            order = torch.randperm(self.n, generator=torch.Generator().manual_seed(int(self.seed) + self.epoch)).tolist()
        return order[self.rank:(self.n // self.world) * self.world:self.world]

    def __iter__(self):
        for i in self.indices():
            sc = synthetic.make_scene(seed=100 + i, **self.kw)
            batch = {k: torch.from_numpy(v) for k, v in sc.items()}
            batch["scene"] = [f"synthetic{i}"]
            batch["view_ids"] = torch.arange(self.kw["n_src_views"] + 1)[None]
            yield batch


class Coach:
    def __init__(self, opts):
        self.opts = opts
        self.n_src_views = opts.n_src_views
        self.device = opts.device
        self.epoch_start = 0
        self.iter_start = 0
        # data-parallel training: the process group train.py (or torchrun) has set up; MNERF_DIST_INIT_ALWAYS makes a one-rank
        # group take the exchange too (tests, timing)
        self.rank, self.world = mdist.rank_world()
        self.distributed = mdist.group_active(always=bool(os.environ.get("MNERF_DIST_INIT_ALWAYS")))

    def build_networks(self):
        self.model = models_dict[self.opts.model](self.opts).to(self.opts.device)  # coach.py:77

    def restore_checkpoint(self):
        """coach.py:127-146.  ``opts.resume``: model, optimizer, scheduler, epoch and iteration from <output_path>/models/latest.pth;
        ``opts.load``: the model's children from that file.  Without either, a TRAINING run (``setup_optimizer`` has been called)
        keeps the module's own initialisation plus the GMFlow weights of ``encoder.pretrain_weight`` if that file exists
        (coach.py:78-81); an inference run gets seeded random weights, so that the tools run offline."""
        path = self.opts.load
        training = hasattr(self, "optim")
        latest = os.path.join(self.opts.output_path, "models", "latest.pth")
        if getattr(self.opts, "resume", False) and training and os.path.isfile(latest):
            state = {k: getattr(self, k) for k in ("optim", "sched") if getattr(self, k, None) is not None}
            self._ckpt_extra = {}
            ep, it = checkpoint.restore_checkpoint(self.model, latest, self.opts.device, resume=True, optims_scheds=state,
                                                   log=self.say, extra=self._ckpt_extra)
            self.epoch_start, self.iter_start = int(ep or 0), int(it or 0)
            self.apply_clip_enc()  # the saved param_groups replaced the live ones
            self.say(f"[coach] resuming from epoch {self.epoch_start} (iteration {self.iter_start})")
            self._check_resumed_world(latest)
        elif path and os.path.isfile(path):
            checkpoint.restore_checkpoint(self.model, path, self.opts.device, log=self.say)
        elif training:
            if getattr(self.opts, "resume", False):
                self.say(f"[coach] no checkpoint at {latest!r}: training starts from scratch")
            pre = self.opts.encoder.pretrain_weight
            if pre and os.path.isfile(pre):
                checkpoint.load_gmflow_checkpoint(self.model.feat_enc, pre, self.opts.device,
                                                  gmflow_n_blocks=self.opts.encoder.num_transformer_layers)
                self.say(f"[coach] encoder initialised from {pre}")
        else:
            self.say(f"[coach] checkpoint {path!r} not found: using seeded random weights (offline run)")
            spec = synthetic.state_dict_spec(n_src_views=self.n_src_views)
            self.model.load_state_dict(synthetic.to_torch(synthetic.seeded_state_dict(spec, 1), self.opts.device))
        if training and self.distributed:
            self.sync_replicas(resumed=bool(getattr(self.opts, "resume", False)))

    def say(self, *args):
        """print on rank 0 only"""
        if self.rank == 0:
            print(*args)

    def _epoch_len(self, world):
        """iterations of one epoch per rank at ``world`` ranks (what len(train_loader) is at the current world size)"""
        if not hasattr(self, "_n_train"):  # a loader that was handed in: only its length per rank is known
            return len(self.train_loader) * self.world // world
        return math.ceil((self._n_train // world) / self._train_batch)

    def _check_resumed_world(self, latest):
        """The checkpoint records the world size it was written at (no key: one process).  `iter` counts optimizer steps and an
        epoch has len(dataset) // W of them per rank, so a checkpoint written in the MIDDLE of an epoch only resumes at its own
        world size; one written at an epoch boundary resumes at any (the new run starts that epoch from its first batch)."""
        saved = int(self._ckpt_extra.get("world_size", 1))
        if saved == self.world or not hasattr(self, "train_loader"):
            return
        if self.iter_start != self.epoch_start * self._epoch_len(saved):
            raise RuntimeError(f"{latest} was written in the middle of epoch {self.epoch_start} (iteration {self.iter_start}) by a run "
                               f"of world size {saved}; this run has world size {self.world}.  A mid-epoch checkpoint resumes only at "
                               "the world size it was written at (resume with the same number of GPUs, or from an epoch-boundary "
                               "checkpoint)")
        self._skip_to = self.epoch_start * len(self.train_loader)  # nothing of epoch `epoch_start` has been done
        if getattr(self, "sched_type", None) == "OneCycleLR":
            # the saved schedule counts the OLD world size's steps per epoch (its total_steps would end early or never): a fresh
            # one for this run's length, advanced to the same epoch
            import warnings
            for g in self.optim.param_groups:
                g.pop("initial_lr", None)
            self._make_sched()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # "lr_scheduler.step() before optimizer.step()": a fast-forward, not training
                for _ in range(self.epoch_start * len(self.train_loader)):  # train_epoch steps it once per batch
                    self.sched.step()

    def sync_replicas(self, resumed=False):
        """Rank 0's model state - and after a resume its optimizer / scheduler state and position - on every rank, so identical
        replicas do not depend on every rank having read the same file or having initialised in the same order."""
        tensors = list(self.model.state_dict().values())
        with torch.no_grad():
            for dtype in sorted({t.dtype for t in tensors}, key=str):
                mdist.broadcast_tensors([t for t in tensors if t.dtype == dtype], src=0)
        if resumed:
            state = None
            if self.rank == 0:
                state = dict(optim=mdist.to_host(self.optim.state_dict()), sched=self.sched.state_dict() if self.sched is not None else None,
                             epoch=self.epoch_start, iter=self.iter_start, skip_to=getattr(self, "_skip_to", None))
            state = mdist.broadcast_object(state, src=0, device=self.opts.device)
            if self.rank != 0:
                self.optim.load_state_dict(state["optim"])
                if self.sched is not None and state["sched"] is not None:
                    self.sched.load_state_dict(state["sched"])
                self.epoch_start, self.iter_start = state["epoch"], state["iter"]
                if state["skip_to"] is not None:
                    self._skip_to = state["skip_to"]
                self.apply_clip_enc()

    def _loader(self, name, cfg, split):
        """One entry of the options' data sections: the on-disk producer where ``root_dir`` exists, synthetic scenes otherwise."""
        train = split == "train"
        root, kind = cfg.get("root_dir"), cfg.get("dataset_name", name)
        if root and os.path.isdir(root) and kind in datasets.datas_dict:  # coach.py:52-69: the on-disk producer
            extra = {k: cfg[k] for k in ("meta_dir", "pairs_file") if cfg.get(k)}  # where the scan / pair lists live
            ds = datasets.datas_dict[kind](root, split, n_views=self.n_src_views, img_wh=cfg.get("img_wh"),
                                           max_len=cfg.get("max_len", -1), scene_list=cfg.get("scene_list"),
                                           test_views_method=cfg.get("test_views_method", "nearest"),
                                           nf_mode=cfg.get("nf_mode", "avg"), eval_mode=cfg.get("eval_mode", "mvsnerf"),
                                           n_add_train_views=cfg.get("n_add_train_views", 2), **extra)
            workers = cfg.get("num_workers", 0)
            if split != "test":
                workers = min(int(workers or 0), 16)
            sampler = None
            if train and self.distributed:  # the order from (seed, epoch) alone, the tail that does not divide dropped
                sampler = torch.utils.data.DistributedSampler(ds, num_replicas=self.world, rank=self.rank, shuffle=True,
                                                              seed=int(self.opts.seed or 0), drop_last=True)
                self._train_sampler = sampler
            if train:
                self._n_train, self._train_batch = len(ds), self.opts.batch_size
            loader = torch.utils.data.DataLoader(ds, shuffle=train and sampler is None, sampler=sampler, num_workers=workers,
                                                 batch_size=self.opts.batch_size, pin_memory=True)
            loader.get_name = ds.get_name
            return loader
        if train and self.distributed:
            scenes = SyntheticScenes(name, cfg, self.n_src_views, shuffle=True, rank=self.rank, world=self.world,
                                     seed=int(self.opts.seed or 0))
            self._n_train, self._train_batch = scenes.n, 1
            return scenes
        scenes = SyntheticScenes(name, cfg, self.n_src_views, shuffle=train)
        if train:
            self._n_train, self._train_batch = scenes.n, 1
        return scenes

    def load_dataset(self, splits=("test",), loaders=None):
        """``loaders``: optional list of iterables of batches (objects with get_name()) for the test split; otherwise
        every ``data_test`` entry whose ``root_dir`` exists is read from disk (datasets.py) and the others are served by the
        synthetic generator at that entry's img_wh.  ``"train"`` / ``"val"`` build ``train_loader`` / ``val_loader`` from
        ``opts.data_train`` / ``opts.data_val`` the same way (training shuffles; at most 16 workers)."""
        if loaders is not None:  # as before: given loaders ARE the test loaders, whatever `splits` says
            self.test_loaders = list(loaders)
        for split in splits:
            if split == "test":
                if loaders is not None:
                    continue
                self.test_loaders = [self._loader(name, cfg, "test") for name, cfg in self.opts.data_test.items()
                                     if cfg is not None]
            elif split in ("train", "val"):
                cfg = getattr(self.opts, f"data_{split}", None)
                if cfg:
                    setattr(self, f"{split}_loader", self._loader(cfg.get("dataset_name", "synthetic"), cfg, split))
            else:
                raise ValueError(f"load_dataset: unknown split {split!r}")

    # ------------------------------------------------------------------ training (coach.py:87-300)

    def setup_optimizer(self):
        """coach.py:87-125: one parameter group per child at ``optim.lr_enc`` / ``optim.lr_dec`` (a rate <= 0 freezes that child:
        per-scene fine-tuning), ``optim.algo`` passed through, ``optim.sched`` with OneCycleLR's extra arguments taken from the run.
        AdamW runs on the fused HIP step (optim.FusedAdamW, ``clip_enc`` as the encoder group's ``max_norm``); with
        ``MNERF_FUSED_OPTIM=0``, and for every other algorithm, the optimizer is ``torch.optim``'s, with ``clip_grad_norm_`` in ``train_iteration``."""
        o = self.opts.optim
        if len(self.opts.gpu_ids) > 1 and not (mdist.group_active(always=True) and self.world == len(self.opts.gpu_ids)):
            raise NotImplementedError(f"gpu_ids = {list(self.opts.gpu_ids)} needs one process per GPU in a process group of that size "
                                      f"(found {'world size ' + str(self.world) if mdist.group_active(always=True) else 'none'}): start "
                                      "the run with `python train.py --gpu_ids=...`, which launches the ranks; the in-process "
                                      "DataParallel form is not built")
        groups, rates = [], []
        self._enc_group = None
        for child, rate in ((self.model.feat_enc, o.lr_enc), (self.model.nerf_dec, o.lr_dec)):
            if rate > 0:
                if child is self.model.feat_enc:
                    self._enc_group = len(groups)
                groups.append(dict(params=list(child.parameters()), lr=rate))
                rates.append(rate)
            else:
                child.requires_grad_(False)
        kind = o.algo.type
        kwargs = {k: v for k, v in o.algo.items() if k != "type"}
        self.fused_optim = kind == "AdamW" and fused_optim_enabled()
        if self.fused_optim:
            from .optim import FusedAdamW
            self.optim = FusedAdamW(groups, **kwargs)
            self.apply_clip_enc()
        else:
            self.optim = getattr(torch.optim, kind)(groups, **kwargs)
        if self.distributed:
            from . import optim as moptim
            self._bucket = moptim.GradBucket() if self.fused_optim else None
            self.say(f"[coach] data-parallel: {self.world} ranks, effective batch {self.world} x {self.opts.batch_size} scenes, "
                     "learning rates not rescaled")
        self.say(f"[coach] {'fused HIP ' if self.fused_optim else ''}{kind} ({', '.join(f'{k}={v}' for k, v in kwargs.items())})")
        self._rates = rates
        self._make_sched()

    def _make_sched(self):
        o = self.opts.optim
        self.sched_type, self.sched = None, None
        if o.get("sched"):
            self.sched_type = o.sched.type
            kwargs = {k: v for k, v in o.sched.items() if k != "type"}
            if self.sched_type == "OneCycleLR":
                assert hasattr(self, "train_loader"), "load the training data first: OneCycleLR needs the number of steps"
                kwargs.update(epochs=self.opts.max_epoch, steps_per_epoch=len(self.train_loader) // self.opts.batch_size,
                              max_lr=self._rates)
            self.sched = getattr(torch.optim.lr_scheduler, self.sched_type)(self.optim, **kwargs)

    def apply_clip_enc(self):
        """Fused path: ``optim.clip_enc`` travels as the encoder group's ``max_norm``.  ``load_state_dict`` replaces the groups by
        the saved ones, and a state written by torch's AdamW or by the reference has no such key: set it again after a restore."""
        if getattr(self, "fused_optim", False) and self._enc_group is not None:
            self.optim.param_groups[self._enc_group]["max_norm"] = self.opts.optim.get("clip_enc")

    def setup_visualizer(self):
        """Scalars always go to <output_path>/scalars.jsonl; a TensorBoard writer is added when ``opts.tb`` is set AND the package
        can be imported."""
        self.tb = None
        if getattr(self.opts, "tb", False) and self.rank == 0:
            try:
                from torch.utils import tensorboard
                self.tb = tensorboard.SummaryWriter(log_dir=self.opts.output_path, flush_secs=10)
            except ImportError:
                print("[coach] tensorboard is not installed: scalars go to scalars.jsonl only")

    def log_scalars(self, scalars, step, split):
        """{tag: value} -> one line per value in scalars.jsonl (+ TensorBoard); rank 0 only"""
        if self.rank != 0:
            return
        with open(os.path.join(self.opts.output_path, "scalars.jsonl"), "a") as f:
            for tag, value in scalars.items():
                f.write(json.dumps({"step": int(step), "split": split, "tag": tag, "value": float(value)}) + "\n")
                if getattr(self, "tb", None) is not None:
                    self.tb.add_scalar(f"{split}/{tag}", float(value), int(step))

    def _every(self, fraction):
        """freq.*_it: a fraction of an epoch -> iterations (coach.py:160-162); <= 0 stays off"""
        return math.ceil(fraction * len(self.train_loader)) if fraction and fraction > 0 else -1

    def train_model(self):
        assert hasattr(self, "optim") and hasattr(self, "train_loader"), "call load_dataset(['train', ...]) and setup_optimizer() first"
        if not hasattr(self, "tb"):
            self.setup_visualizer()
        f = self.opts.freq
        self.it, self.ep = self.iter_start, self.epoch_start
        self.val_it, self.test_it, self.ckpt_it = self._every(f.val_it), self._every(f.test_it), self._every(f.ckpt_it)
        self.timer = edict(start=time.time(), it_mean=None)
        if getattr(self.opts, "sanity_check", False) and self.it == 0 and self.val_it > 0:
            self.rank0_then_barrier(lambda: self.validate_model(first_only=True))
        self.say(f"[coach] training: epochs {self.epoch_start}..{self.opts.max_epoch - 1}, {len(self.train_loader)} iterations each")
        for self.ep in range(self.epoch_start, self.opts.max_epoch):
            self.train_epoch()
        if getattr(self, "tb", None) is not None:
            self.tb.flush()
            self.tb.close()
        self.say(f"[coach] training done: {self.it} iterations")

    def train_epoch(self):
        f = self.opts.freq
        self.model.train()
        loss, n = None, len(self.train_loader)  # per rank: `it` counts optimizer steps
        for owner in (self.train_loader, getattr(self, "_train_sampler", None)):
            if hasattr(owner, "set_epoch"):
                owner.set_epoch(self.ep)  # the same order on every rank, from (seed, epoch)
        skip_to = getattr(self, "_skip_to", self.iter_start)
        for bi, batch in enumerate(self.train_loader):
            if getattr(self.opts, "resume", False) and self.ep * n + bi < skip_to:
                continue  # iterations the resumed run has already done
            var = self._to_device(batch)
            loss = self.train_iteration(var)
            if self.sched_type == "OneCycleLR":
                self.sched.step()
        if loss is not None and f.log_ep > 0 and (self.ep + 1) % f.log_ep == 0 and self.rank == 0:
            lr = self.get_cur_lrates()
            timer = getattr(self, "timer", None)
            shown = float(loss.all.detach()) if getattr(self, "_loss_mean", None) is None else float(self._loss_mean[0])  # mean over ranks
            print(f"[coach] epoch {self.ep + 1}: loss {shown:.5f}  lr enc {lr['enc']:.3e} dec {lr['dec']:.3e}"
                  + (f"  {timer.it_mean * 1e3:.1f} ms / iteration" if timer is not None else ""))
        if self.sched_type is not None and self.sched_type != "OneCycleLR":
            self.sched.step()
        if f.val_ep > 0 and (self.ep + 1) % f.val_ep == 0:
            self.validate_model()  # every rank: the evaluation is sharded
        if hasattr(self, "test_loaders") and self.ep >= f.test_ep_start and f.test_ep > 0 and (self.ep + 1) % f.test_ep == 0:
            self.test_model(save_images=bool(getattr(self.opts, "save_test_image", False)))
            self.model.train()
        if f.ckpt_ep > 0 and (self.ep + 1) % f.ckpt_ep == 0:
            self.rank0_then_barrier(lambda: self.save_checkpoint(ep=self.ep + 1, it=self.it, backup_ckpt=True))

    def rank0_then_barrier(self, work):
        """Checkpoints and the sanity check are rank 0's alone (validation and tests are sharded over the ranks: ``_evaluate``); the
        other ranks wait at a barrier before the next iteration, whose collective would otherwise wait for it."""
        if self.rank == 0:
            work()
        if self.distributed:
            mdist.barrier(always=True)

    def exchange_gradients(self, side=None):
        """Between backward and clip + step: every gradient becomes the mean over the ranks (sum, then times fp32(1 / W)), and the
        ``side`` values (the iteration's loss) come back as their mean in the same collective."""
        params = [p for g in self.optim.param_groups for p in g["params"]]
        if getattr(self, "_bucket", None) is not None:
            return self._bucket.reduce(params, side, always=True)
        from .optim import reduce_gradients_torch
        return reduce_gradients_torch(params, side, always=True)

    def train_iteration(self, var):
        """coach.py:215-243: zero_grad, mode='train' forward, loss, backward, clip, step - and the per-iteration bookkeeping."""
        t0 = time.time()
        clip = self.opts.optim.get("clip_enc")
        if self.fused_optim and clip is not None and self._enc_group is not None:  # the fused step clips inside (max_norm)
            if self.optim.param_groups[self._enc_group].get("max_norm") != clip:
                raise RuntimeError("the encoder group of the fused optimizer has lost its max_norm (optim.clip_enc): "
                                   "a load_state_dict() replaced the parameter groups; call Coach.apply_clip_enc()")
        self.optim.zero_grad(set_to_none=True)
        pred = self.model(var, mode="train")
        loss = self.compute_loss(pred, var, mode="train")
        loss.all = None
        for k, w in self.opts.loss_weight.items():
            if w is not None and k in loss:
                term = loss[k] if w == 1 else w * loss[k]
                loss.all = term if loss.all is None else loss.all + term
        loss.all.backward()
        mean = None
        if self.distributed:  # slot 0: the loss; then its terms, in the order the scalars are logged
            terms = [k for k in loss if k != "all"]
            mean = self._loss_mean = self.exchange_gradients(torch.stack([loss.all.detach()] + [loss[k].detach() for k in terms]))
        if clip is not None and not self.fused_optim:
            torch.nn.utils.clip_grad_norm_(self.model.feat_enc.parameters(), clip)
        self.optim.step()

        self.it += 1
        if getattr(self, "timer", None) is not None:
            dt = time.time() - t0
            self.timer.it_mean = dt if self.timer.it_mean is None else 0.99 * self.timer.it_mean + 0.01 * dt
        f = self.opts.freq
        if f.scalar > 0 and self.it % f.scalar == 0 and self.rank == 0:
            if mean is not None:  # the mean over the ranks: it rode in the gradient bucket, no collective of its own
                scalars = {f"loss_{k}": float(v) for k, v in zip(terms, mean[1:])}
            else:
                scalars = {f"loss_{k}": float(v.detach()) for k, v in loss.items() if k != "all"}
            scalars.update({f"lrate_{k}": v for k, v in self.get_cur_lrates().items()})
            self.log_scalars(scalars, self.it, "train")
        if getattr(self, "ckpt_it", -1) > 0 and self.it % self.ckpt_it == 0:
            self.rank0_then_barrier(lambda: self.save_checkpoint(ep=self.ep, it=self.it, backup_ckpt=False))
        if getattr(self, "val_it", -1) > 0 and self.it % self.val_it == 0:
            self.validate_model()  # every rank: the evaluation is sharded
        if getattr(self, "test_it", -1) > 0 and self.it % self.test_it == 0 and hasattr(self, "test_loaders"):
            self.test_model(save_images=bool(getattr(self.opts, "save_test_image", False)))
            self.model.train()
        return loss

    def compute_loss(self, pred, src, mode=None):
        """coach.py:245-259: the L2 loss of the rendered colours against the target view's pixels (at ``pred.ray_idx`` when the
        mode draws random rays) or against ``train_color``.  On the fused path it is one HIP launch (autograd.l2_loss)."""
        loss = edict()
        if "train_color" in src:
            gt = src["train_color"]
        else:
            b, n_views, c = src.images.shape[:3]
            assert n_views == self.n_src_views + 1, "the last view of a batch is the target view"
            gt = src.images[:, -1].reshape(b, c, -1).permute(0, 2, 1)  # [B, H*W, 3]
            if getattr(self.opts.nerf, f"rand_rays_{mode}", None) and mode == "train":
                gt = gt[:, pred.ray_idx]
        if self.opts.loss_weight.render is not None:
            if getattr(self, "fused_optim", False):
                from .autograd import l2_loss
                loss.render = l2_loss(pred.rgb, gt.contiguous())
            else:
                loss.render = ((pred.rgb.contiguous() - gt) ** 2).mean()
        return loss

    def get_cur_lrates(self):
        o = self.opts.optim
        enc, dec = o.lr_enc, o.lr_dec
        if getattr(self, "sched", None) is not None:
            last = self.sched.get_last_lr()
            if enc > 0:
                enc = last[0]
            if dec > 0:
                dec = last[-1]
        return dict(enc=enc, dec=dec)

    def save_checkpoint(self, ep=0, it=0, backup_ckpt=True):
        """coach.py:290-300: {model, optim, sched, epoch, iter} -> <output_path>/models/latest.pth (+ ep{E}_it{I}.pth without the
        optimizer and scheduler state when ``backup_ckpt``); a data-parallel run adds ``world_size``."""
        ckpt = dict(model=self.model.state_dict(), optim=self.optim.state_dict())
        if self.world > 1:  # no key: written by one process
            ckpt["world_size"] = self.world
        if getattr(self, "sched", None) is not None:
            ckpt["sched"] = self.sched.state_dict()
        return checkpoint.save_checkpoint(self.opts.output_path, ckpt, ep=ep, it=it, backup_ckpt=backup_ckpt)

    # ------------------------------------------------------------------ evaluation (coach.py:316-453)

    def _eval_world(self):
        """(rank, world) of a sharded evaluation: the process group's when it has more than one rank, else (0, 1)"""
        return (self.rank, self.world) if mdist.group_active() else (0, 1)

    def _own_batches(self, loader, rank, world):
        """-> (global batch index, batch) of the batches of ``loader`` that belong to ``rank`` (metrics.batch_owner: bi % world).  An
        on-disk DataLoader in its sequential order is rebuilt over a batch sampler of the rank's indices, so that no rank reads
        another rank's files; every other loader is iterated and the other ranks' batches are skipped."""
        if world == 1:
            yield from enumerate(loader)
            return
        data = torch.utils.data
        if isinstance(loader, data.DataLoader) and isinstance(loader.sampler, data.SequentialSampler) and loader.batch_size:
            n, bs = len(loader.dataset), loader.batch_size
            n_batches = (n + bs - 1) // bs if not loader.drop_last else n // bs
            mine = metrics.rank_batches(n_batches, rank, world)
            if not mine:
                return
            own = data.DataLoader(loader.dataset, batch_sampler=[list(range(bi * bs, min((bi + 1) * bs, n))) for bi in mine],
                                  num_workers=loader.num_workers, pin_memory=loader.pin_memory)
            yield from zip(mine, own)
            return
        for bi, batch in enumerate(loader):
            if metrics.batch_owner(bi, world) == rank:
                yield bi, batch

    def _to_device(self, batch):
        """a loader's batch as an edict with its tensors on the run's device"""
        return edict({k: (v.to(self.opts.device) if torch.is_tensor(v) else v) for k, v in batch.items()})

    def _stem(self, batch, bi):
        """`<scene>_view<tgt>_src<ids>` of batch element bi: the reference's name of its video (coach.py:507-509)"""
        ids = [int(x) for x in batch["view_ids"][bi]] if "view_ids" in batch else list(range(self.n_src_views + 1))
        scene = batch["scene"][bi] if "scene" in batch else f"scene{bi}"
        return f"{scene}_view{ids[-1]:02d}_src" + "_".join(f"{x:02d}" for x in ids[:self.n_src_views])

    def _path_mode(self, name, default=None):
        """The video path of test set ``name``: llff spiral, colmap by its config, dtu / blender interpolate.  The reference has no
        rule for the other sets (ibrnet, tnt, ...; coach.py:480-481): ``default`` where one is given, else an exception."""
        if name == "llff":
            return "spiral"
        if name == "colmap":
            return getattr(getattr(self.opts.data_test, "colmap", {}), "render_path_mode", "interpolate")
        if name in ("dtu", "blender"):
            return "interpolate"
        if default is None:
            raise Exception(f"Unknown dataset for rendering video {name}")
        return default

    def _require_pinhole(self, what, batch=None):
        """Scored evaluation compares with the batch's target image, a pinhole photograph: another camera model (the option
        nerf.render_camera, or a batch.tgt_camera) has no ground truth to be scored against - test_model_video renders those."""
        spec = batch.get("tgt_camera") if batch is not None else getattr(self.opts.nerf, "render_camera", None)
        name = spec.get("model") if isinstance(spec, dict) else spec
        if name not in (None, "", "pinhole"):
            raise ValueError(f"{what}: the target camera is {name!r}, but the ground truth it would be scored against is a pinhole "
                             "image; render other camera models with nerf.render_video (test_model_video) or MatchNeRF.forward")

    def _evaluate(self, loader, mode, mask_of, on_frame=None, lpips_fn=None, first_only=False, shard=True, device_lpips=None,
                  depth_panels=False):
        """Render this rank's batches of ``loader`` in ``mode`` and score them -> rows float64 [n, 5] of ALL ranks' images in the
        order one process evaluates them: (batch index, image within the batch, PSNR, SSIM, LPIPS or NaN).
        On CUDA with ``metrics.device_metrics_enabled()`` PSNR / SSIM are rows of ``metrics.DeviceEval`` (csrc/metrics.hip) and reach
        the host in ONE copy after the last batch; a frame goes to the host only for ``on_frame(batch, bi, i, pred, gt)`` (images to
        write) or a host LPIPS callable ``lpips_fn``.  With ``device_lpips`` (a ``metrics.DeviceLPIPS``; CUDA path only) LPIPS is a
        fifth column of the same rows (csrc/lpips.hip) and no frame leaves the device for it.  Otherwise every frame is scored on
        the host (``metrics.psnr`` / ``EvalTools``).
        ``mask_of(gt_depth)`` -> the depth the invalid mask (depth == 0) comes from, or None for the 80 % centre crop.
        With a process group of more than one rank (``shard``), the ranks' rows travel in one ragged ``dist.gather_blocks``.
        ``depth_panels`` (vis_depth): ``on_frame`` gets a sixth argument, the frame's colour-mapped depth [h, w, 3] uint8
        (``_depth_panels``)."""
        self._require_pinhole("evaluation")
        rank, world = self._eval_world() if shard else (0, 1)
        on_device = str(self.opts.device).startswith("cuda") and metrics.device_metrics_enabled()
        dev = metrics.DeviceEval(device_lpips) if on_device else None
        host_rows, lpips_of = [], {}
        for bi, batch in self._own_batches(loader, rank, world):
            if first_only and bi > 0:
                break
            var = self._to_device(batch)
            gt_depth = var.pop("depth") if "depth" in var else None  # forward overwrites 'depth'
            self._require_pinhole("evaluation", var)
            b, _, _, h, w = var.images.shape
            # scored against a ground truth of the batch's size: the option nerf.render_hw (videos) is not read here, and a batch
            # that names another grid cannot be scored
            if tuple(int(v) for v in var.get("tgt_hw", (h, w))) != (h, w):
                raise ValueError(f"evaluation: batch.tgt_hw={tuple(var.tgt_hw)} differs from the ground truth's size {(h, w)}")
            var.tgt_hw = (h, w)
            var = self.model(var, mode=mode)
            depth = mask_of(gt_depth)
            frames = None
            panels = self._depth_panels(var.depth.reshape(b, h, w), batch["near_fars"][:, -1]) if depth_panels and on_frame is not None \
                else None
            if dev is None or on_frame is not None or lpips_fn is not None:
                frames = (var.rgb.reshape(b, h, w, 3).cpu().numpy(), var.images[:, -1].permute(0, 2, 3, 1).cpu().numpy())
            if dev is not None:
                dev.add(bi, var.rgb.reshape(b, h * w, 3).contiguous(), var.images[:, -1],
                        None if depth is None else (depth.reshape(b, h, w) == 0))
            for i in range(b if frames is not None else 0):
                pred, gt = frames[0][i], frames[1][i]
                mask = None if depth is None else (depth[i].cpu().numpy() == 0)
                if dev is None or lpips_fn is not None:
                    tools = metrics.EvalTools(lpips_fn=lpips_fn)
                    tools.set_inputs(pred, gt, mask)
                if dev is None:
                    host_rows.append([bi, i, metrics.psnr(pred, gt, mask), tools.get_metrics(["SSIM"])["SSIM"], np.nan])
                if lpips_fn is not None:
                    lpips_of[(bi, i)] = tools.get_metrics(["LPIPS"])["LPIPS"]
                if on_frame is not None:
                    on_frame(batch, bi, i, pred, gt, *(() if panels is None else (panels[i],)))
        if dev is not None:
            keys, got = dev.finish()  # the one copy of this loader
            last = got[:, 4:5] if dev.lpips is not None else np.full((len(keys), 1), np.nan)
            rows = np.concatenate([keys.astype(np.float64), got[:, :2], last], 1)
        else:
            rows = np.asarray(host_rows, np.float64).reshape(-1, 5)
        for j in range(len(rows) if lpips_of else 0):
            rows[j, 4] = lpips_of.get((int(rows[j, 0]), int(rows[j, 1])), np.nan)
        return metrics.gather_rows(rows, device=self.opts.device) if world > 1 else metrics.merge_rows(rows)

    def _depth_panels(self, depth, near_fars):
        """vis_depth: depth [B, ..., h, w] float32 on the device -> uint8 [B, ..., h, w, 3] on the host, colour-mapped on the device
        (hip.depth_colormap: the arithmetic of the reference's visualize_depth, misc/utils.py:323-341) with minmax = element b's
        ``near_fars[b]``, as coach.py:404-408 / 497-505 pass it."""
        from . import hip
        near_fars = torch.as_tensor(near_fars).detach().cpu().numpy()
        return np.stack([hip.depth_colormap(depth[b].contiguous().float(), float(near_fars[b, 0]), float(near_fars[b, 1])).cpu().numpy()
                         for b in range(depth.shape[0])], 0)

    @torch.no_grad()
    def validate_model(self, first_only=False):
        """coach.py:316-366: every batch of ``val_loader`` rendered in mode='val'; mean PSNR / SSIM to the scalars, prediction | ground
        truth strips to <output_path>/validation/.  In a data-parallel run every rank calls this: batch bi is rendered, scored and its
        strip written by rank bi % W, rank 0 logs and prints the one-process report (``first_only``, the sanity check, is rank 0's
        alone and runs no collective)."""
        assert hasattr(self, "val_loader"), "load_dataset(['val']) first"
        self._require_pinhole("validate_model")
        from PIL import Image
        self.model.eval()
        out_dir = os.path.join(self.opts.output_path, "validation")
        os.makedirs(out_dir, exist_ok=True)
        name = self.val_loader.get_name()
        it = getattr(self, "it", 0)

        def strip(batch, bi, i, pred, gt):
            scene = batch["scene"][i] if "scene" in batch else f"{name}{bi}"
            vis = (np.concatenate([pred, gt], 1).clip(0, 1) * 255).astype("uint8")
            Image.fromarray(vis).save(os.path.join(out_dir, f"{scene}_{bi:03d}_{i}_it{it}.jpg"))

        rows = self._evaluate(self.val_loader, "val", lambda d: d if (d is not None and "dtu" in name) else None, on_frame=strip,
                              first_only=first_only, shard=not first_only)
        psnrs, ssims = [float(v) for v in rows[:, 2]], [float(v) for v in rows[:, 3]]
        self.log_scalars({"PSNR": np.mean(psnrs), "SSIM": np.mean(ssims)}, it, "val")
        self.say(f"[coach] validation at iteration {it}: PSNR {np.mean(psnrs):.2f} over {len(psnrs)} images")
        self.model.train()
        return dict(PSNR=psnrs, SSIM=ssims)

    @torch.no_grad()
    def test_model(self, save_images=False, **kwargs):
        """coach.py:368-453 -> {dataset: {image_id: psnr}}; the results file also lists SSIM and, when the two weight files of the
        `lpips` package are on disk (metrics.load_lpips: $MNERF_LPIPS_VGG16 / $MNERF_LPIPS_LIN or torch hub's cache), LPIPS.
        ``save_images`` writes prediction | ground truth strips, with vis_depth depth | prediction | ground truth (coach.py:404-408).
        With a process group of more than one rank every rank calls this and renders batch bi when bi % W is its rank; rank 0 alone
        writes the results files and prints, every rank returns the one-process report and writes the images of its own share."""
        self._require_pinhole("test_model")
        self.model.eval()
        lpips_fn, device_lpips = None, None
        if str(self.opts.device).startswith("cuda") and metrics.device_metrics_enabled() and metrics.device_lpips_enabled():
            try:  # LPIPS as a fifth column of the device rows (csrc/lpips.hip); the streams are packed once per coach
                paths = (os.environ.get("MNERF_LPIPS_VGG16"), os.environ.get("MNERF_LPIPS_LIN"), os.environ.get("TORCH_HOME"))
                if getattr(self, "_device_lpips", (None, None))[0] != paths:
                    self._device_lpips = (paths, metrics.DeviceLPIPS(self.opts.device))
                device_lpips = self._device_lpips[1]
            except FileNotFoundError:
                pass
        else:
            try:
                lpips_fn = metrics.load_lpips(device=self.opts.device)
            except FileNotFoundError:
                pass
        has_lpips = lpips_fn is not None or device_lpips is not None
        out_root = os.path.join(self.opts.output_path, "test")
        os.makedirs(out_root, exist_ok=True)
        report = {}
        for loader in self.test_loaders:
            name = loader.get_name()
            self.model.nerf_setbg_opaque = (name == "blender")  # coach.py:382-383

            def save(batch, bi, i, pred, gt, depth_vis=None, name=name):
                from PIL import Image
                vis = (np.concatenate([pred, gt], 1).clip(0, 1) * 255).astype("uint8")
                if depth_vis is not None:  # vis_depth: depth | pred | gt (coach.py:404-408)
                    vis = np.concatenate([depth_vis, vis], 1)
                Image.fromarray(vis).save(os.path.join(out_root, f"{name}_{bi:03d}_{i}.png"))

            rows = self._evaluate(loader, "test", lambda d: d, on_frame=save if save_images else None, lpips_fn=lpips_fn,
                                  device_lpips=device_lpips, depth_panels=bool(getattr(self.opts, "vis_depth", False)))
            self.model.nerf_setbg_opaque = False
            report[name] = {f"{name}_{int(r[0]):03d}_{int(r[1])}": float(r[2]) for r in rows}
            ssims = [float(r[3]) for r in rows]
            lpipss = [float(r[4]) if has_lpips else None for r in rows]
            vals = list(report[name].values())
            if self.rank == 0:
                with open(os.path.join(out_root, f"0results_{name}.txt"), "w") as f:
                    for (k, v), sv, lv in zip(report[name].items(), ssims, lpipss):
                        f.write(f"{k}: PSNR {v:.4f} SSIM {sv:.4f}" + (f" LPIPS {lv:.4f}" if lv is not None else "") + "\n")
                    f.write(f"mean PSNR {np.mean(vals):.4f} SSIM {np.mean(ssims):.4f}" +
                            (f" LPIPS {np.mean(lpipss):.4f}" if has_lpips else "") + "\n")
            self.say(f"[coach] {name}: mean PSNR {np.mean(vals):.2f} over {len(vals)} images")
        return report

    @torch.no_grad()
    def test_model_video(self, **kwargs):
        """coach.py:455-529: every batch of every test set rendered along its video path (dtu / blender / colmap-by-config:
        interpolate, llff: spiral; white background for blender), written under <output_path>/test_videos/<set>/ as the reference
        names them: `<scene>_view<tgt>_src<ids>.gif` at 12 fps when nerf.save_gif, `..._f<i>.jpg` frames when nerf.save_frames, and
        the strip of source views `<name>.jpg` (PIL instead of imageio; the reference's .mp4 needs scikit-video / ffmpeg, neither in
        this image, and is skipped).  With vis_depth every frame is rgb | depth (coach.py:497-505).  Frames have the rendered size: the views', or nerf.render_hw (optionally
        supersampled: nerf.render_ssaa), through the batch's pinhole camera or the model nerf.render_camera names (fisheye / sphere
        with nerf.render_fov degrees, ortho with nerf.render_ortho_width world units: MatchNeRF.target_camera).  Returns {set: frames [F,h,w,3] uint8 of its FIRST batch element}."""
        from PIL import Image
        self.model.eval()
        out_root = os.path.join(self.opts.output_path, "test_videos")
        videos = {}
        for loader in self.test_loaders:
            name = loader.get_name()
            out_dir = os.path.join(out_root, name)
            os.makedirs(out_dir, exist_ok=True)
            mode = self._path_mode(name)
            self.model.nerf_setbg_opaque = (name == "blender")
            n_frames = int(self.opts.nerf.video_n_frames)
            for batch in loader:
                var = self._to_device(batch)
                # (coach.py:487-488 passes opts.nerf.render_video; this method IS the video test, so a config that leaves the
                # switch off still gets the frames - and is told so once)
                if not getattr(self.opts.nerf, "render_video", True) and not getattr(self, "_warned_render_video", False):
                    import warnings
                    warnings.warn("test_model_video: nerf.render_video is off in the options; rendering the video path anyway")
                    self._warned_render_video = True
                if getattr(self.opts, "vis_depth", False) and not getattr(self, "_warned_vis_depth", False):
                    import warnings
                    warnings.warn("test_model_video: the .mp4 container (skvideo, coach.py:511-525) is not written: frames / GIF / "
                                  "source strip only")
                    self._warned_vis_depth = True
                b = var.images.shape[0]
                h, w = self.model.target_grid(var, "test", self.model.extract_poses(var)[0], var.images.shape[-2:])[1]  # nerf.render_hw
                var = self.model(var, mode="test", render_video=True, render_path_mode=mode)
                # forward returns the reference's frame-major layout [n_frames * B, h*w, 3] at the rendered size
                frames = (var.rgb.reshape(n_frames, b, h, w, 3).clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
                if getattr(self.opts, "vis_depth", False):  # rgb | depth, the depth panel on the right (coach.py:497-505)
                    # (forward hands video frames over on the host: the depths go back for the colour map, [B, F, h, w])
                    depth = var.depth.reshape(n_frames, b, h, w).to(self.opts.device).transpose(0, 1)
                    panels = self._depth_panels(depth, batch["near_fars"][:, -1])
                    frames = np.concatenate([frames, panels.transpose(1, 0, 2, 3, 4)], axis=3)
                for bi in range(b):
                    clip = frames[:, bi]
                    videos.setdefault(name, clip)
                    stem = self._stem(batch, bi)
                    if getattr(self.opts.nerf, "save_frames", False):
                        for fi, fr in enumerate(clip):
                            Image.fromarray(fr).save(os.path.join(out_dir, f"{stem}_f{fi}.jpg"))
                    if getattr(self.opts.nerf, "save_gif", False):
                        imgs = [Image.fromarray(fr) for fr in clip]
                        imgs[0].save(os.path.join(out_dir, f"{stem}.gif"), save_all=True, append_images=imgs[1:], duration=1000 // 12, loop=0)
                    src = (var.images[bi, :self.n_src_views].permute(0, 2, 3, 1).cpu().numpy() * 255).astype("uint8")
                    Image.fromarray(np.concatenate(list(src), axis=1)).save(os.path.join(out_dir, f"{stem}.jpg"))
            self.model.nerf_setbg_opaque = False
        return videos

    @torch.no_grad()
    def export_geometry(self, views=None, **kwargs):
        """Every batch of every test set as a coloured point cloud (MatchNeRF.export_points: depth maps rendered at the fusion poses,
        kept where other poses confirm them) -> <output_path>/geometry/<set>/<stem>.ply, binary little-endian, float xyz + uchar rgb,
        with the stems of ``test_model_video``; with vis_depth also one colour-mapped depth map per fusion view, <stem>_depth<k>.png
        (minmax = the target's near_fars, as the reference's depth panels).  ``views``: 'sources' | 'path' (default: the option
        nerf.export_geometry, else 'sources'); thresholds from nerf.fuse_px_tol / fuse_rel_tol / fuse_min_opacity / fuse_min_views
        where given.  With the option nerf.export_mesh also <stem>_mesh.ply next to each cloud: the triangle mesh of the same maps
        (``fusion.mesh``: TSDF fusion + marching tetrahedra; float xyz + uchar rgb vertices and a face list), with nerf.mesh_resolution /
        mesh_voxel / mesh_trunc / mesh_min_weight where given, cleaned up by nerf.mesh_min_component / mesh_min_component_fraction
        (small connected components dropped), nerf.mesh_smooth (rounds of Taubin smoothing) and nerf.mesh_decimate (quadric
        vertex clustering with cells of that many voxels, applied last) where given; with nerf.mesh_sparse the volume is
        brick-sparse (``fusion.mesh(sparse=True)``: the same surface, the rows in brick order, for resolutions past the dense grid);
        with nerf.mesh_normals the vertices also carry
        float nx ny nz (``fusion.vertex_normals`` of the mesh that is written).  With nerf.mesh_texture=B also <stem>_mesh.obj, .mtl and
        .png next to <stem>_mesh.ply: the same mesh with a texture atlas of B x B blocks baked from the views (``fusion.texture``;
        nerf.mesh_texture_best / mesh_texture_power / mesh_texture_rel_tol where given; nerf.mesh_texture_from = 'render' (default)
        | 'images': the source photographs instead of their re-renderings, with 'sources' views only); <stem>_mesh.ply is the same
        bytes with or without it; nerf.mesh_texture_visibility = 'views' (default) | 'mesh': test a texel's visibility against the
        mesh's own depth.  With nerf.mesh_report also <stem>_mesh_report.json: ``fusion.mesh_report`` of the written mesh against the
        maps it was fused from (per view and pooled: coverage, spurious, relative depth error, PSNR); with nerf.mesh_preview also
        <stem>_mesh_preview_<k>.png per fusion view, the shaded mesh next to the field's frame (``mesh | render``, 2 w x h).  Both
        shade from the atlas when one was baked, from the vertex colours otherwise.  One process (not sharded).
        Returns {set: [path of every .ply, of every .obj after its mesh's .ply, then the report and the previews of that mesh]}."""
        import json

        from PIL import Image

        from . import fusion
        self.model.eval()
        views = views or getattr(self.opts.nerf, "export_geometry", None) or "sources"
        if views is True:
            views = "sources"
        fuse_args = {arg: getattr(self.opts.nerf, name) for arg, name in (("px_tol", "fuse_px_tol"), ("rel_tol", "fuse_rel_tol"),
                                                                          ("min_opacity", "fuse_min_opacity"),
                                                                          ("min_consistent", "fuse_min_views"))
                     if getattr(self.opts.nerf, name, None) is not None}
        mesh_args = None
        if getattr(self.opts.nerf, "export_mesh", None):
            mesh_args = {arg: getattr(self.opts.nerf, name) for arg, name in (("resolution", "mesh_resolution"), ("voxel", "mesh_voxel"),
                                                                              ("trunc", "mesh_trunc"), ("min_weight", "mesh_min_weight"),
                                                                              ("min_component", "mesh_min_component"),
                                                                              ("min_component_fraction", "mesh_min_component_fraction"),
                                                                              ("smooth", "mesh_smooth"), ("decimate", "mesh_decimate"),
                                                                              ("sparse", "mesh_sparse"))
                         if getattr(self.opts.nerf, name, None) is not None}
            fusion._decimate_cell("nerf.mesh_decimate", mesh_args.get("decimate", 0.0))  # refused before anything is rendered
            fusion._sparse_flag("nerf.mesh_sparse", mesh_args.get("sparse", False))
            mesh_args.update({arg: getattr(self.opts.nerf, name) for arg, name in (("texture", "mesh_texture"), ("texture_best", "mesh_texture_best"),
                                                                                   ("texture_power", "mesh_texture_power"),
                                                                                   ("texture_vis_rel_tol", "mesh_texture_rel_tol"),
                                                                                   ("texture_visibility", "mesh_texture_visibility"))
                              if getattr(self.opts.nerf, name, None) is not None})
            fusion._visibility("nerf.mesh_texture_visibility", mesh_args.get("texture_visibility", "views"))
            texture_from = getattr(self.opts.nerf, "mesh_texture_from", None) or "render"
            self.model.check_texture("nerf.mesh_texture", mesh_args.get("texture", 0), mesh_args.get("texture_power", 2), texture_from, views)
        mesh_normals = bool(getattr(self.opts.nerf, "mesh_normals", None))
        mesh_report = mesh_args is not None and bool(getattr(self.opts.nerf, "mesh_report", None))
        mesh_preview = mesh_args is not None and bool(getattr(self.opts.nerf, "mesh_preview", None))
        out_root = os.path.join(self.opts.output_path, "geometry")
        written = {}
        for loader in self.test_loaders:
            name = loader.get_name()
            out_dir = os.path.join(out_root, name)
            os.makedirs(out_dir, exist_ok=True)
            mode = self._path_mode(name, default="interpolate")
            self.model.nerf_setbg_opaque = (name == "blender")
            for batch in loader:
                var = self._to_device(batch)
                clouds, maps = self.model.export_points(var, views=views, render_path_mode=mode, return_maps=True, **fuse_args)
                panels = self._depth_panels(maps.depth, batch["near_fars"][:, -1]) if getattr(self.opts, "vis_depth", False) else None
                for bi, cloud in enumerate(clouds):
                    stem = self._stem(batch, bi)
                    path = os.path.join(out_dir, f"{stem}.ply")
                    n = fusion.write_ply(path, cloud)
                    written.setdefault(name, []).append(path)
                    self.say(f"[coach] {name}: {n} points -> {path}")
                    if mesh_args is not None:  # the surface of the same maps, fused into a TSDF volume
                        photos = self.model.source_colours(var)[bi] if mesh_args.get("texture", 0) and texture_from == "images" else None
                        vertices, faces, *textured = fusion.mesh(maps.views[bi], maps.depth[bi], maps.opacity[bi], maps.rgb[bi], maps.hw,
                                                                 bool(self.opts.nerf.legacy_coord), texture_rgbs=photos, **mesh_args,
                                                                 **fuse_args)
                        path = os.path.join(out_dir, f"{stem}_mesh.ply")
                        vertex_normals = fusion.vertex_normals(vertices, faces) if mesh_normals else None
                        fusion.write_ply(path, vertices, faces, vertex_normals)
                        written[name].append(path)
                        self.say(f"[coach] {name}: {vertices.shape[0]} vertices, {faces.shape[0]} triangles -> {path}")
                        if textured:
                            path = os.path.join(out_dir, f"{stem}_mesh.obj")
                            fusion.write_obj(path, vertices, faces, *textured, vertex_normals)
                            written[name].append(path)
                            self.say(f"[coach] {name}: a {textured[1].shape[1]} x {textured[1].shape[0]} atlas -> {path}")
                        if mesh_report or mesh_preview:
                            shading = dict(atlas=textured[1] if textured else None, block=mesh_args.get("texture", 0) if textured else 0)
                            legacy = bool(self.opts.nerf.legacy_coord)
                        if mesh_report:
                            report = fusion.mesh_report(vertices, faces, maps.views[bi], maps.depth[bi], maps.opacity[bi], maps.rgb[bi],
                                                        maps.hw, legacy, min_opacity=fuse_args.get("min_opacity", 0.5), **shading)
                            path = os.path.join(out_dir, f"{stem}_mesh_report.json")
                            with open(path, "w") as f:
                                json.dump(report, f, indent=1)
                            written[name].append(path)
                            pooled = report["pooled"]
                            self.say(f"[coach] {name}: the mesh covers {pooled['coverage']:.3f} of the field, {pooled['spurious']:.3f} of it "
                                     f"is spurious, depth within {pooled['depth_rel_mean']:.4f}, {pooled['psnr']:.2f} dB -> {path}")
                        if mesh_preview:
                            h, w = maps.hw
                            rgba = fusion.render_mesh(vertices, faces, fusion._open_views(maps.views[bi]), maps.hw, legacy, **shading)[0]
                            both = torch.cat([rgba[..., :3], maps.rgb[bi].reshape(-1, h, w, 3)], 2)  # mesh | render
                            both = (both.nan_to_num().clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
                            for k, panel in enumerate(both):
                                path = os.path.join(out_dir, f"{stem}_mesh_preview_{k}.png")
                                Image.fromarray(panel).save(path)
                                written[name].append(path)
                    for k in range(panels.shape[1] if panels is not None else 0):
                        Image.fromarray(panels[bi, k]).save(os.path.join(out_dir, f"{stem}_depth{k}.png"))
            self.model.nerf_setbg_opaque = False
        return written
