"""``FusedAdamW``: ``torch.optim.AdamW`` whose ``step()`` is three HIP launches for all tensors of all groups
(csrc/optim.hip: gradient norm per group -> clip + AdamW), whatever the number of tensors.

Only ``step()`` is overridden: state initialisation, ``state_dict()`` / ``load_state_dict()``, ``param_groups`` and the scheduler
hooks are torch's, so a checkpoint written by ``torch.optim.AdamW`` (state ``step`` / ``exp_avg`` / ``exp_avg_sq``) resumes here and
the other way round.  A per-group ``max_norm`` key carries ``clip_grad_norm_`` (None / <= 0: no clipping): the clip coefficient
is formed on the device from the device-side norm, the clipped values are left in ``.grad`` as ``clip_grad_norm_`` leaves them.

The kernels write through raw pointers, so after the launch the version counter of every updated parameter is bumped: the
weight-stream caches of this package (CondNeRF, TransformerPacker, the conv packs, the encoder graph) are keyed on ``_version``.

No CPU fallback (CPU parameters raise ``hip.MnerfError`` at ``step()``), no amsgrad / maximize / capturable / differentiable,
fp32 contiguous dense tensors only - each raises instead of taking another path."""
import numpy as np
import torch

from . import hip

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


class FusedAdamW(torch.optim.AdamW):
    def __init__(self, params, *args, **kwargs):
        if kwargs.get("fused"):
            raise ValueError("FusedAdamW: `fused=True` selects torch's own fused kernel; leave it unset")
        super().__init__(params, *args, **kwargs)
        self._check_groups()
        for group in self.param_groups:
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise TypeError(f"FusedAdamW: parameters must be float32, got {p.dtype}")
        self._key = None       # identity of the tensors the cached table was built for
        self._table = None     # numpy record array, one mnerf_optim_row per tensor with a gradient
        self._sent = None      # bytes of the table the device holds
        self._pinned = []      # ring of (pinned uint8 tensor, event recorded after its copy)
        self._dev = None       # (rows uint8, workspace float32, sumsq float32) on the parameters' device

    def _check_groups(self):
        if len(self.param_groups) > hip.OPTIM_MAX_GROUPS:
            raise ValueError(f"FusedAdamW: {len(self.param_groups)} parameter groups, at most {hip.OPTIM_MAX_GROUPS}")
        for group in self.param_groups:
            for k in _UNSUPPORTED:
                if group.get(k):
                    raise ValueError(f"FusedAdamW: {k}=True is not supported (use torch.optim.AdamW)")
            if torch.is_tensor(group["lr"]) and group["lr"].is_cuda:
                raise ValueError("FusedAdamW: a CUDA tensor `lr` would need a device->host copy per step; use a float")

    @staticmethod
    def _check_tensor(p):
        g = p.grad
        if g.is_sparse:
            raise RuntimeError("FusedAdamW does not support sparse gradients")
        if not p.is_cuda or not g.is_cuda:
            raise hip.MnerfError(f"FusedAdamW: the HIP kernels need CUDA tensors, got a parameter on {p.device} "
                                 "(there is no CPU fallback)")
        if p.dtype != torch.float32 or g.dtype != torch.float32:
            raise TypeError(f"FusedAdamW: float32 parameters and gradients only, got {p.dtype} / {g.dtype}")
        if not p.is_contiguous() or not g.is_contiguous():
            raise ValueError(f"FusedAdamW: parameter {tuple(p.shape)} or its gradient is not contiguous")
        if g.device != p.device or g.shape != p.shape:
            raise ValueError(f"FusedAdamW: gradient {tuple(g.shape)} on {g.device} vs parameter {tuple(p.shape)} on {p.device}")

    def _pinned_buffer(self, nbytes):
        """A pinned staging buffer whose last copy has run (no wait: a buffer still in flight is left alone and the ring grows)."""
        for slot in self._pinned:
            if slot[0].numel() >= nbytes and slot[1].query():
                return slot
        slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        self._pinned.append(slot)
        return slot

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        per_group = [[p for p in group["params"] if p.grad is not None] for group in self.param_groups]
        params = [p for ps in per_group for p in ps]
        if not params:
            return loss
        state = self.state
        if any(not state.get(p) for p in params):
            # first step of some tensor: everything is checked BEFORE torch's own state initialisation touches anything
            for p in params:
                self._check_tensor(p)
            for group in self.param_groups:
                self._init_group(group, [], [], [], [], [], [])
        sts = [state[p] for p in params]
        steps = [st["step"] for st in sts]
        exp_avgs = [st["exp_avg"] for st in sts]
        exp_avg_sqs = [st["exp_avg_sq"] for st in sts]
        device = params[0].device

        key = tuple(map(id, params)) + tuple(map(id, exp_avgs)) + tuple(map(id, exp_avg_sqs))
        if key != self._key:
            for p in params:
                self._check_tensor(p)
            if any(p.device != device for p in params):
                raise ValueError("FusedAdamW: all parameters must live on one device")
            for m, v, p in zip(exp_avgs, exp_avg_sqs, params):
                for s in (m, v):
                    if s.dtype != torch.float32 or not s.is_contiguous() or s.device != device or s.shape != p.shape:
                        raise ValueError("FusedAdamW: optimizer state must be contiguous float32 on the parameter's device")
            t = np.zeros(len(params), np.dtype(hip.OptimRow))
            t["numel"] = [p.numel() for p in params]
            if (t["numel"] <= 0).any():
                raise ValueError("FusedAdamW: empty parameter tensor")
            blocks = (t["numel"] + hip.OPTIM_CHUNK - 1) // hip.OPTIM_CHUNK
            t["block_begin"] = np.cumsum(blocks) - blocks
            t["group"] = [gi for gi, ps in enumerate(per_group) for _ in ps]
            t["exp_avg"] = [m.data_ptr() for m in exp_avgs]
            t["exp_avg_sq"] = [v.data_ptr() for v in exp_avg_sqs]
            if int(t["group"].min()) < 0 or int(t["group"].max()) >= len(self.param_groups) or int(t["block_begin"][0]) != 0:
                raise RuntimeError("FusedAdamW: malformed row table (group index / block prefix)")  # the kernel only clamps
            self._table, self._key, self._sent = t, key, None
            self._refs = (params, exp_avgs, exp_avg_sqs)  # keeps the ids of the key from being reused
            self._n_blocks = int(blocks.sum())
            self._group_blocks = [int(blocks[t["group"] == gi].sum()) for gi in range(len(per_group))]
        elif not all(g.dtype == torch.float32 and g.is_contiguous() and g.device == device and g.numel() == p.numel()
                     for p, g in ((p, p.grad) for p in params)):
            for p in params:  # same tensors as last step, only the gradients are new: name the one that is off
                self._check_tensor(p)
        # torch keeps `step` per parameter on the CPU: advancing and reading it is no device sync
        torch._foreach_add_(steps, 1)
        step_vals = np.asarray([s.item() for s in steps], np.float64)
        t = self._table
        t["param"] = [p.data_ptr() for p in params]
        t["grad"] = [p.grad.data_ptr() for p in params]
        at = 0
        for group, ps in zip(self.param_groups, per_group):
            b1, b2 = (float(b) for b in group["betas"])
            s = step_vals[at:at + len(ps)]
            t["bias_correction1"][at:at + len(ps)] = 1.0 - b1 ** s
            t["bias_correction2_sqrt"][at:at + len(ps)] = np.sqrt(1.0 - b2 ** s)
            at += len(ps)
        groups = hip.optim_groups([(group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"],
                                    group.get("max_norm"), nb) for group, nb in zip(self.param_groups, self._group_blocks)])
        clips = any((group.get("max_norm") or 0) > 0 for group in self.param_groups)

        n_rows, nbytes = len(params), t.nbytes
        with torch.cuda.device(device):
            if self._dev is None or self._dev[0].device != device or self._dev[0].numel() < nbytes or self._dev[1].numel() < self._n_blocks:
                self._dev = (torch.empty(nbytes, dtype=torch.uint8, device=device), torch.empty(self._n_blocks, device=device),
                             torch.zeros(hip.OPTIM_MAX_GROUPS, device=device))
                self._sent = None
            rows, workspace, sumsq = self._dev
            raw = t.view(np.uint8).reshape(-1)
            if self._sent is None or not np.array_equal(raw, self._sent):  # nothing moved: the device already holds this table
                slot = self._pinned_buffer(nbytes)
                slot[0].numpy()[:nbytes] = raw
                rows[:nbytes].copy_(slot[0][:nbytes], non_blocking=True)
                slot[1].record()
                self._sent = raw.copy()
            if clips:
                hip.grad_sumsq(rows, n_rows, self._n_blocks, groups, workspace, sumsq)
            hip.adamw_step(rows, n_rows, self._n_blocks, groups, sumsq if clips else None)
        self.last_sumsq = sumsq if clips else None  # device tensor [groups]: squared gradient norms of this step (no sync to keep it)

        # the kernels wrote through raw pointers: tell autograd and every cache keyed on _version
        touched = list(params)
        for group, ps in zip(self.param_groups, per_group):
            if (group.get("max_norm") or 0) > 0:
                touched += [p.grad for p in ps]
        torch.autograd.graph.increment_version(touched)
        return loss
