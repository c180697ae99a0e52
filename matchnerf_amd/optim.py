"""``FusedAdamW``: ``torch.optim.AdamW`` whose ``step()`` is three HIP launches for all tensors of all groups
(csrc/optim.hip: gradient norm per group -> clip + AdamW), whatever the number of tensors.

Only ``step()`` is overridden: state initialisation, ``state_dict()`` / ``load_state_dict()``, ``param_groups`` and the scheduler
hooks are torch's, so a checkpoint written by ``torch.optim.AdamW`` (state ``step`` / ``exp_avg`` / ``exp_avg_sq``) resumes here and
the other way round.  A per-group ``max_norm`` key carries ``clip_grad_norm_`` (None / <= 0: no clipping): the clip coefficient
is formed on the device from the device-side norm, the clipped values are left in ``.grad`` as ``clip_grad_norm_`` leaves them.

The kernels write through raw pointers, so after the launch the version counter of every updated parameter is bumped: the
weight-stream caches of this package (CondNeRF, TransformerPacker, the conv packs, the encoder graph) are keyed on ``_version``.

No CPU fallback (CPU parameters raise ``hip.MnerfError`` at ``step()``), no amsgrad / maximize / capturable / differentiable,
fp32 contiguous dense tensors only - each raises instead of taking another path.

``GradBucket``: the gradient exchange of data-parallel training over the same row table (``RowTable``, shared with the step):
pack every gradient into one bucket (one launch) -> ONE sum over the ranks -> unpack times fp32(1 / world) (one launch).
``reduce_gradients_torch`` is the same exchange with torch's ops, for the optimizers that are torch's."""
import hashlib

import numpy as np
import torch
import torch.distributed as dist

from . import hip
from .dist import group_active

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


def check_tensor(p, who="FusedAdamW"):
    g = p.grad
    if g.is_sparse:
        raise RuntimeError(f"{who} does not support sparse gradients")
    if not p.is_cuda or not g.is_cuda:
        raise hip.MnerfError(f"{who}: the HIP kernels need CUDA tensors, got a parameter on {p.device} "
                             "(there is no CPU fallback)")
    if p.dtype != torch.float32 or g.dtype != torch.float32:
        raise TypeError(f"{who}: float32 parameters and gradients only, got {p.dtype} / {g.dtype}")
    if not p.is_contiguous() or not g.is_contiguous():
        raise ValueError(f"{who}: parameter {tuple(p.shape)} or its gradient is not contiguous")
    if g.device != p.device or g.shape != p.shape:
        raise ValueError(f"{who}: gradient {tuple(g.shape)} on {g.device} vs parameter {tuple(p.shape)} on {p.device}")


def row_blocks(numels):
    """numel list -> (block_begin of every row, n_blocks): a tensor is cut into chunks of hip.OPTIM_CHUNK elements"""
    numels = np.asarray(numels, np.int64)
    blocks = (numels + hip.OPTIM_CHUNK - 1) // hip.OPTIM_CHUNK
    return np.cumsum(blocks) - blocks, int(blocks.sum())


class RowTable:
    """The device table of mnerf_optim_row records that the kernels of csrc/optim.hip walk: built once per set of tensors,
    refreshed with the pointers of the step, staged through a ring of pinned buffers and sent only when a byte of it moved."""

    def __init__(self, who):
        self.who = who
        self.key = None       # identity of the tensors the cached table was built for
        self.table = None     # numpy record array, one mnerf_optim_row per tensor with a gradient
        self.n_blocks = 0
        self._sent = None     # bytes of the table the device holds
        self._pinned = []     # ring of (pinned uint8 tensor, event recorded after its copy)
        self._rows = None     # uint8 tensor on the parameters' device

    def rebuild(self, key, params, groups=None, exp_avgs=None, exp_avg_sqs=None):
        """A fresh table for ``params`` (every one checked); ``groups``: the group index of every row, sorted."""
        device = params[0].device
        for p in params:
            check_tensor(p, self.who)
        if any(p.device != device for p in params):
            raise ValueError(f"{self.who}: all parameters must live on one device")
        t = np.zeros(len(params), np.dtype(hip.OptimRow))
        t["numel"] = [p.numel() for p in params]
        if (t["numel"] <= 0).any():
            raise ValueError(f"{self.who}: empty parameter tensor")
        t["block_begin"], self.n_blocks = row_blocks(t["numel"])
        if groups is not None:
            t["group"] = groups
        if exp_avgs is not None:
            t["exp_avg"] = [m.data_ptr() for m in exp_avgs]
            t["exp_avg_sq"] = [v.data_ptr() for v in exp_avg_sqs]
        if int(t["block_begin"][0]) != 0:
            raise RuntimeError(f"{self.who}: malformed row table (block prefix)")  # the kernels only clamp
        self.table, self.key, self._sent = t, key, None
        self._refs = (params, exp_avgs, exp_avg_sqs)  # keeps the ids of the key from being reused
        return t

    def check_gradients(self, params):
        device = params[0].device
        if not all(g.dtype == torch.float32 and g.is_contiguous() and g.device == device and g.numel() == p.numel()
                   for p, g in ((p, p.grad) for p in params)):
            for p in params:  # same tensors as last step, only the gradients are new: name the one that is off
                check_tensor(p, self.who)

    def _pinned_buffer(self, nbytes):
        """A pinned staging buffer whose last copy has run (no wait: a buffer still in flight is left alone and the ring grows)."""
        for slot in self._pinned:
            if slot[0].numel() >= nbytes and slot[1].query():
                return slot
        slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        self._pinned.append(slot)
        return slot

    def send(self, params):
        """The table with this step's parameter and gradient pointers on the device -> the uint8 tensor of rows.  Call under
        ``torch.cuda.device(device)``."""
        t = self.table
        t["param"] = [p.data_ptr() for p in params]
        t["grad"] = [p.grad.data_ptr() for p in params]
        device, nbytes = params[0].device, t.nbytes
        if self._rows is None or self._rows.device != device or self._rows.numel() < nbytes:
            self._rows = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._sent = None
        raw = t.view(np.uint8).reshape(-1)
        if self._sent is None or not np.array_equal(raw, self._sent):  # nothing moved: the device already holds this table
            slot = self._pinned_buffer(nbytes)
            slot[0].numpy()[:nbytes] = raw
            self._rows[:nbytes].copy_(slot[0][:nbytes], non_blocking=True)
            slot[1].record()
            self._sent = raw.copy()
        return self._rows


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
        self._rows = RowTable("FusedAdamW")
        self._dev = None       # (workspace float32, sumsq float32) on the parameters' device

    def _check_groups(self):
        if len(self.param_groups) > hip.OPTIM_MAX_GROUPS:
            raise ValueError(f"FusedAdamW: {len(self.param_groups)} parameter groups, at most {hip.OPTIM_MAX_GROUPS}")
        for group in self.param_groups:
            for k in _UNSUPPORTED:
                if group.get(k):
                    raise ValueError(f"FusedAdamW: {k}=True is not supported (use torch.optim.AdamW)")
            if torch.is_tensor(group["lr"]) and group["lr"].is_cuda:
                raise ValueError("FusedAdamW: a CUDA tensor `lr` would need a device->host copy per step; use a float")

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
                check_tensor(p)
            for group in self.param_groups:
                self._init_group(group, [], [], [], [], [], [])
        sts = [state[p] for p in params]
        steps = [st["step"] for st in sts]
        exp_avgs = [st["exp_avg"] for st in sts]
        exp_avg_sqs = [st["exp_avg_sq"] for st in sts]
        device = params[0].device

        rt = self._rows
        key = tuple(map(id, params)) + tuple(map(id, exp_avgs)) + tuple(map(id, exp_avg_sqs))
        if key != rt.key:
            for m, v, p in zip(exp_avgs, exp_avg_sqs, params):
                for s in (m, v):
                    if s.dtype != torch.float32 or not s.is_contiguous() or s.device != device or s.shape != p.shape:
                        raise ValueError("FusedAdamW: optimizer state must be contiguous float32 on the parameter's device")
            group_of = [gi for gi, ps in enumerate(per_group) for _ in ps]
            t = rt.rebuild(key, params, group_of, exp_avgs, exp_avg_sqs)
            blocks = (t["numel"] + hip.OPTIM_CHUNK - 1) // hip.OPTIM_CHUNK
            self._n_blocks = rt.n_blocks
            self._group_blocks = [int(blocks[t["group"] == gi].sum()) for gi in range(len(per_group))]
        else:
            rt.check_gradients(params)
        # torch keeps `step` per parameter on the CPU: advancing and reading it is no device sync
        torch._foreach_add_(steps, 1)
        step_vals = np.asarray([s.item() for s in steps], np.float64)
        t = rt.table
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

        n_rows = len(params)
        with torch.cuda.device(device):
            if self._dev is None or self._dev[0].device != device or self._dev[0].numel() < self._n_blocks:
                self._dev = (torch.empty(self._n_blocks, device=device), torch.zeros(hip.OPTIM_MAX_GROUPS, device=device))
            workspace, sumsq = self._dev
            rows = rt.send(params)
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


# ---------------------------------------------------------------------------------------------- data-parallel gradient exchange


def mean_scale(world):
    """the fp32 value 1 / world that both exchanges MULTIPLY the summed gradients by (never a division: at world = 3 the two
    would round differently), as a Python float that fp32 holds exactly"""
    return float(np.float32(1.0) / np.float32(world))


def agree_on_rows(numels, who, error=None):
    """Every rank must walk the same row list: (n_rows, n_blocks, a hash of the numel list, whether this rank's own checks failed)
    are exchanged with one small collective and ALL ranks raise if any differs or failed - a rank that raised alone would leave the
    others waiting in the next collective.  ``error``: what this rank's own checks raised; it is re-raised here, after the exchange.
    Run before EVERY exchange: the set of tensors that hold a gradient, or a gradient's layout, can change on one rank alone.  The
    price is one 32-byte all-gather and, over RCCL, one wait for the device per iteration."""
    numels = [] if error is not None else [int(n) for n in numels]
    digest = hashlib.sha256(np.asarray(numels, np.int64).tobytes()).digest()
    mine = torch.tensor([len(numels), row_blocks(numels)[1] if numels else 0, int.from_bytes(digest[:7], "little"),
                         int(error is not None)], dtype=torch.int64)
    world, rank = dist.get_world_size(), dist.get_rank()
    if dist.get_backend() != "gloo":
        mine = mine.cuda()
    everyone = torch.empty(world * 4, dtype=torch.int64, device=mine.device)
    dist.all_gather_into_tensor(everyone, mine)
    everyone = everyone.cpu().reshape(world, 4)
    if error is not None:
        raise error
    if bool(everyone[:, 3].any()) or not bool((everyone == everyone[0]).all()):
        raise RuntimeError(f"{who}: the ranks disagree on the gradients to exchange, or a rank refused its own; (tensors, chunks, hash "
                           f"of the sizes, refused) per rank: {[tuple(r) for r in everyone.tolist()]} (this is rank {rank})")


class GradBucket:
    """``reduce(params, side)``: the gradients of ``params`` become their mean over the ranks, ``side`` (a few device floats, e.g.
    the loss) comes back as its mean - pack (one launch), one sum of the bucket over the ranks, unpack * fp32(1 / world) (one launch).
    The bucket is hip.grad_bucket_floats(n_blocks) floats: every tensor starts on a chunk boundary (about 6 % padding at the model's 153
    tensors, 20 MB).  Every rank applies the same operations to the same summed values, so replicas that start equal stay equal."""

    def __init__(self):
        self._rows = RowTable("GradBucket")
        self._bucket = None

    @torch.no_grad()
    def reduce(self, params, side=None, always=False):
        params = [p for p in params if p.grad is not None]
        if not group_active(always):
            return side
        world = dist.get_world_size()
        rt = self._rows
        key = tuple(map(id, params))
        err = None
        try:  # a rank whose own tensors are refused still takes part in the agreement, and raises after it
            if not params:
                raise ValueError("GradBucket: no parameter has a gradient")
            if key != rt.key:
                rt.rebuild(key, params)
            else:
                rt.check_gradients(params)
        except Exception as e:  # noqa: BLE001
            err, rt.key = e, None
        agree_on_rows([p.numel() for p in params], "GradBucket", err)
        device = params[0].device
        n_rows, n_blocks = len(params), rt.n_blocks
        if side is not None:
            side = side.detach().reshape(-1).float().contiguous()
        with torch.cuda.device(device):
            floats = hip.grad_bucket_floats(n_blocks)
            if self._bucket is None or self._bucket.device != device or self._bucket.numel() != floats:
                self._bucket = torch.empty(floats, device=device)
            rows = rt.send(params)
            hip.grad_pack(rows, n_rows, n_blocks, self._bucket, side)
            sum_over_ranks(self._bucket)
            out = torch.empty_like(side) if side is not None else None
            hip.grad_unpack(rows, n_rows, n_blocks, self._bucket, mean_scale(world), out)
        torch.autograd.graph.increment_version([p.grad for p in params])  # written through raw pointers
        return out


def sum_over_ranks(flat):
    """In place: ``flat`` (1-d float32) becomes the sum of every rank's ``flat``, the same bits on every rank.  Over RCCL it is one
    all_reduce on the device buffer.  Over gloo (the dry-run transport: several ranks on one GPU) device tensors are staged through
    the host as in dist.gather_blocks, and the ranks' buffers are gathered and added in rank order: gloo's ring all_reduce adds the
    ranks in an order that depends on an element's POSITION in the buffer (measured at three ranks), so the padded bucket and the dense
    flat buffer of the torch path would differ in the last bit; added in rank order they are comparable exactly."""
    if dist.get_backend() != "gloo":
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        return flat
    world = dist.get_world_size()
    host = flat.cpu() if flat.is_cuda else flat
    if world <= 2:  # a + b = b + a: nothing to order
        dist.all_reduce(host, op=dist.ReduceOp.SUM)
    else:
        everyone = host.new_empty(world * host.numel())
        dist.all_gather_into_tensor(everyone, host.contiguous())
        parts = everyone.reshape(world, -1)
        host = parts[0].clone()
        for r in range(1, world):
            host += parts[r]
    if flat.is_cuda or host is not flat:
        flat.copy_(host)
    return flat


@torch.no_grad()
def reduce_gradients_torch(params, side=None, always=False):
    """The exchange of ``GradBucket.reduce`` with torch's ops (MNERF_FUSED_OPTIM=0, or an optimizer other than AdamW; CPU tensors
    work): flatten -> sum over the ranks -> times the same fp32 scalar -> copy back.  Same bits as the kernel path."""
    from torch._utils import _flatten_dense_tensors, _unflatten_dense_tensors
    params = [p for p in params if p.grad is not None]
    if not group_active(always):
        return side
    agree_on_rows([p.numel() for p in params], "reduce_gradients_torch")
    grads = [p.grad for p in params]
    if side is not None:
        side = side.detach().reshape(-1).to(grads[0].dtype)
    flat = _flatten_dense_tensors(grads + ([side] if side is not None else []))
    sum_over_ranks(flat)
    flat.mul_(mean_scale(dist.get_world_size()))
    parts = _unflatten_dense_tensors(flat, grads + ([side] if side is not None else []))
    torch._foreach_copy_(grads, list(parts[:len(grads)]))
    return parts[-1].clone() if side is not None else None
