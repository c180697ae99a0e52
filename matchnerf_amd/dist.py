"""Multi-GPU sharding of the render path: one process per GPU, RCCL over xGMI.

Rays of a frame — and whole target views — are independent given the (replicated) weights
and source-view feature maps, so the path shards with NO collective inside
the kernels.  By default (``encoder="recompute"``) each rank re-runs the encoder on the shared source
views; ``encoder="shared"`` (``encode_shared``) splits it by view and by view pair and gathers tokens and maps.
Measured on one MI355X, the slowest share at 8 ranks costs 2.90 ms against 3.56 ms for the whole
encoder at 3 views (one pair per rank underfills the attention grid), 5.1 ms against 32.1 ms at 10 views; the
gathers then deliver 0.20 GB / 1.14 GB per rank, whose xGMI time is not measured.  Each rank renders its own
slice, and ONE collective returns the rendered tiles: ``all_gather_into_tensor`` of ``[rays_local, 5]`` fp32
(rgb, depth, opacity) — 6.5 MB per 512x640 frame, latency-bound on xGMI.
The reference has only ``nn.DataParallel`` (coach.py:83-85), which at batch_size 1
degenerates to one GPU.
"""
import os

import torch
import torch.distributed as dist


def init_from_env(backend=None):
    """torchrun-style env (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*) -> (rank, world, device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if "MNERF_FORCE_DEVICE" in os.environ:  # dry runs of the N>1 path on a 1-GPU box (with gloo)
        local = int(os.environ["MNERF_FORCE_DEVICE"])
    backend = backend or os.environ.get("MNERF_DIST_BACKEND")
    use_cuda = torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(local)
    device = torch.device(f"cuda:{local}" if use_cuda else "cpu")
    if (world > 1 or os.environ.get("MNERF_DIST_INIT_ALWAYS")) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend or ("nccl" if use_cuda else "gloo"), rank=rank, world_size=world)
    return rank, world, device


def shard_range(n_items, rank, world):
    """Contiguous, balanced partition of range(n_items): -> (begin, count); the first
    ``n_items % world`` ranks take one extra item."""
    base, extra = divmod(n_items, world)
    begin = rank * base + min(rank, extra)
    return begin, base + (1 if rank < extra else 0)


def shard_rows(height, width, rank, world):
    """Row-tile partition of one frame -> (first_ray, n_rays) in row-major pixel order."""
    r0, nr = shard_range(height, rank, world)
    return r0 * width, nr * width


def gather_blocks(local, counts=None, dim=0, always=False):
    """All ranks receive the concatenation along ``dim`` of every rank's ``local`` block, in rank order.  ``counts`` = per-rank
    sizes along ``dim``; when omitted they are exchanged first (one int per rank), so ragged blocks (a rank with more, fewer or
    no rows) never reach the collective with mismatched sizes.  Blocks are padded to the largest and trimmed after the
    collective, so a single all_gather_into_tensor suffices; every other dimension must agree across ranks.
    ``always``: run the collectives also in a one-rank group (tests: the RCCL calls on device tensors execute on a
    single GPU exactly as they do on eight)."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not always):
        return local
    world, rank = dist.get_world_size(), dist.get_rank()
    on_host = dist.get_backend() == "gloo"
    rows = local.movedim(dim, 0)
    if counts is None:
        mine = torch.tensor([rows.shape[0]], dtype=torch.int64, device="cpu" if on_host else local.device)
        allc = torch.empty(world, dtype=torch.int64, device=mine.device)
        dist.all_gather_into_tensor(allc, mine)
        counts = [int(c) for c in allc.tolist()]
    # every rank must raise together: a rank that raised alone would leave the others waiting in the collective
    bad_here = len(counts) != world or counts[rank] != rows.shape[0]
    flag = torch.tensor([1 if bad_here else 0], dtype=torch.int32, device="cpu" if on_host else local.device)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    if int(flag.item()):
        raise ValueError(f"gather_blocks: rank {rank} holds {rows.shape[0]} rows along dim {dim}, counts={list(counts)} "
                         f"(world {world})" + ("" if bad_here else " [another rank's block disagrees with its count]"))
    width = max(counts)
    if width == 0:  # nothing anywhere
        return local
    send = rows
    if rows.shape[0] != width:
        send = rows.new_zeros((width,) + tuple(rows.shape[1:]))
        send[:rows.shape[0]] = rows
    if send.is_cuda and on_host:  # dry-run path (gloo with GPU tensors): stage through the host
        host = send.contiguous().cpu()
        out_h = host.new_empty((world * width,) + tuple(host.shape[1:]))
        dist.all_gather_into_tensor(out_h, host)
        out = out_h.to(send.device)
    else:
        out = rows.new_empty((world * width,) + tuple(rows.shape[1:]))
        dist.all_gather_into_tensor(out, send.contiguous())
    if any(c != width for c in counts):
        out = torch.cat([out[r * width:r * width + counts[r]] for r in range(world)], 0)
    return out.movedim(0, dim)


def gather_tiles(local, counts=None, always=False):
    """All ranks receive the concatenation of every rank's ``local`` [n_r, C] tile, in rank order: ``gather_blocks`` along
    the first dimension (``counts`` = per-rank row counts, exchanged first when omitted)."""
    return gather_blocks(local, counts, 0, always)


def encoder_partition(n_views, world):
    """Shares of the encoder when ranks split it (``encode_shared``): -> list over ranks of (views, pairs), two contiguous,
    balanced ranges - the source views whose backbone the rank runs and the view pairs (``camera.pair_list`` order) whose
    transformer and up-sampler it runs.  Counts differ by at most one; a rank may get an empty range (3 pairs over 8 ranks)."""
    n_pairs = n_views * (n_views - 1) // 2
    parts = []
    for r in range(world):
        v0, nv = shard_range(n_views, r, world)
        p0, npr = shard_range(n_pairs, r, world)
        parts.append((range(v0, v0 + nv), range(p0, p0 + npr)))
    return parts


def encode_shared(model, images):
    """``model.get_img_feat(images)`` with the encoder split over the ranks instead of repeated on each: every rank runs the
    backbone of its share of the views (``encoder_partition``), ONE ragged all_gather gives all ranks every view's tokens, every
    rank runs the transformer and up-sampler of its share of the view pairs, and one ragged all_gather per scale returns the
    pair-major maps.  -> the list of two maps [B, P, 2, h_s, w_s, 128] of ``get_img_feat`` (same layout, dtype, contiguity),
    identical on every rank.  No process group or one rank: ``get_img_feat`` itself.  Inference only."""
    if torch.is_grad_enabled():
        raise RuntimeError("encode_shared: the shared encoder is inference only (no backward through the gathers); "
                           "call it under torch.no_grad()")
    n_views = model.n_src_views
    splits, wo_self_attn = model.opts.encoder.attn_splits_list, model.opts.encoder.wo_self_attn
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return model.get_img_feat(images, attn_splits_list=splits, cur_n_src_views=n_views)
    images = images[:, :n_views]
    parts = encoder_partition(n_views, dist.get_world_size())
    views, pairs = parts[dist.get_rank()]
    enc = model.feat_enc
    tok = gather_blocks(enc.backbone_tokens(images, views, splits), [len(v) for v, _ in parts], dim=1)
    maps = enc.pair_maps(tok, pairs, splits, wo_self_attn)
    return [gather_blocks(m, [len(p) for _, p in parts], dim=1).contiguous() for m in maps]


def _source_features(model, ref_images, encoder):
    if encoder == "recompute":
        return model.get_img_feat(ref_images, cur_n_src_views=model.n_src_views)
    if encoder == "shared":
        return encode_shared(model, ref_images)
    raise ValueError(f"encoder={encoder!r}: expected 'recompute' or 'shared'")


def _require_pinhole(model, batch, mode, who):
    """Sharded rendering has no ray-bundle form: a target camera other than the batch's pinhole one (``batch.tgt_camera`` or the
    option nerf.render_camera, ``MatchNeRF.target_camera``) is refused on every rank, before the encoder and any collective."""
    spec = model.target_camera(batch, mode)
    if spec is not None:
        raise NotImplementedError(f"{who}: a {spec['model']} target camera renders a ray bundle, which is not sharded; "
                                  "render it on one GPU (MatchNeRF.forward)")


def render_frame_sharded(model, batch, mode="test", encoder="recompute"):
    """BASELINE config[3], row-tile form: every rank renders its contiguous band of rows of the target view through the HIP
    path, and ONE all_gather returns the [rays_local, 5] tiles (rgb, depth, opacity) to all ranks.  -> edict(rgb [B,HW,3],
    depth [B,HW,1], opacity [B,HW,1]) of the target grid (``model.target_grid``: the views' size unless the batch or the options name another), identical on every rank and bit-identical to the unsharded ``model.render`` from the
    same feature maps (rays are independent; tests/test_dist_gpu.py).  ``encoder``: "recompute" - every rank encodes the
    (replicated) source views itself; "shared" - the ranks split the encoder (``encode_shared``, inference only)."""
    from .edict import EasyDict as edict
    if encoder not in ("recompute", "shared"):
        raise ValueError(f"encoder={encoder!r}: expected 'recompute' or 'shared'")
    rank, world = rank_world()
    _require_pinhole(model, batch, mode, "render_frame_sharded")
    ref_images = batch.images[:, :model.n_src_views]
    feats = _source_features(model, ref_images, encoder)
    tgt_pose, ref_poses = model.extract_poses(batch)
    b = ref_images.shape[0]
    tgt_pose, (h, w), ssaa = model.target_grid(batch, mode, tgt_pose, ref_images.shape[-2:])  # rows of the TARGET grid are split
    first, n = shard_rows(h, w, rank, world)
    out = model.render(model.opts, tgt_pose, ray_range=(first, n), mode=mode, ref_poses=ref_poses, ref_images=ref_images,
                       ref_feats_list=feats, tgt_hw=(h, w), ssaa=ssaa)
    tile = torch.cat([out.rgb, out.depth, out.opacity], -1).permute(1, 0, 2).reshape(n, b * 5)   # rows = rays
    full = gather_tiles(tile, [shard_rows(h, w, r, world)[1] for r in range(world)])
    full = full.reshape(h * w, b, 5).permute(1, 0, 2)
    return edict(rgb=full[..., :3].contiguous(), depth=full[..., 3:4].contiguous(), opacity=full[..., 4:5].contiguous())


def render_views_sharded(model, batch, poses, mode="test", encoder="shared"):
    """BASELINE config[3] as the reference runs it: ONE source set (``batch``'s source views and cameras) and a list of target
    ``poses`` (dicts of extrinsics / intrinsics / near_fars, e.g. a ``model.get_video_rendering_path`` result; their intrinsics are
    the batch's target camera's, which ``model.target_grid`` moves to ``nerf.render_hw`` where that option applies).  The poses are
    split contiguously over the ranks (``shard_range``), each rank renders its own full frames with ``model.render``, and one
    ragged all_gather of [n_local_poses * B * HW, 5] returns them.  -> the reference's frame-major edict(rgb [F*B, HW, 3],
    depth [F*B, HW, 1], opacity [F*B, HW, 1]) (matchnerf.py:62-70), identical on every rank.  ``encoder``: as in
    ``render_frame_sharded``."""
    from .edict import EasyDict as edict
    if encoder not in ("recompute", "shared"):
        raise ValueError(f"encoder={encoder!r}: expected 'recompute' or 'shared'")
    rank, world = rank_world()
    _require_pinhole(model, batch, mode, "render_views_sharded")
    ref_images = batch.images[:, :model.n_src_views]
    feats = _source_features(model, ref_images, encoder)
    _, ref_poses = model.extract_poses(batch)
    b = ref_images.shape[0]
    h, w = model.target_grid(batch, mode, None, ref_images.shape[-2:])[1]  # frames of the TARGET grid are gathered
    spans = [shard_range(len(poses), r, world) for r in range(world)]
    first, n = spans[rank]
    frames = []
    for pose in poses[first:first + n]:
        pose, tgt_hw, ssaa = model.target_grid(batch, mode, pose, ref_images.shape[-2:])
        out = model.render(model.opts, pose, mode=mode, ref_poses=ref_poses, ref_images=ref_images, ref_feats_list=feats,
                           tgt_hw=tgt_hw, ssaa=ssaa)
        frames.append(torch.cat([out.rgb, out.depth, out.opacity], -1))   # [B, HW, 5]
    local = torch.stack(frames, 0).reshape(n * b * h * w, 5) if frames else ref_images.new_zeros((0, 5))
    full = gather_tiles(local, [c * b * h * w for _, c in spans]).reshape(len(poses) * b, h * w, 5)
    return edict(rgb=full[..., :3].contiguous(), depth=full[..., 3:4].contiguous(), opacity=full[..., 4:5].contiguous())


def group_active(always=False):
    """a process group exists and has more than one rank (``always``: one rank counts too)"""
    return dist.is_initialized() and (dist.get_world_size() > 1 or always)


def rank_world():
    return (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)


def reseed(seed, rank):
    """Data-parallel training: rank r reseeds torch's CPU and device generators with ``seed + r`` once the options are processed,
    so the ranks draw different rays and stratified offsets (the order of the scenes must NOT come from these generators)."""
    torch.manual_seed(int(seed) + int(rank))
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(int(seed) + int(rank))


def broadcast_tensors(tensors, src=0):
    """Rank ``src``'s values of ``tensors`` (one dtype) into every rank's, in ONE broadcast of the flattened list; device tensors
    are staged through the host over gloo."""
    from torch._utils import _flatten_dense_tensors, _unflatten_dense_tensors
    if not tensors or not dist.is_initialized():
        return
    flat = _flatten_dense_tensors([t.detach() for t in tensors])
    if flat.is_cuda and dist.get_backend() == "gloo":
        host = flat.cpu()
        dist.broadcast(host, src=src)
        flat = host.to(flat.device)
    else:
        dist.broadcast(flat, src=src)
    if dist.get_rank() != src:
        for t, v in zip(tensors, _unflatten_dense_tensors(flat, tensors)):
            t.detach().copy_(v)


def to_host(obj):
    """a nested dict / list / tuple with its tensors on the CPU (what travels through broadcast_object must not name a device)"""
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_host(v) for v in obj)
    return obj


def broadcast_object(obj, src=0, device=None):
    """``obj`` of rank ``src`` (anything torch can pickle) on every rank"""
    if not dist.is_initialized():
        return obj
    box = [obj]
    dist.broadcast_object_list(box, src=src, device=None if dist.get_backend() == "gloo" else device)
    return box[0]


def barrier(always=False):
    if dist.is_initialized() and (dist.get_world_size() > 1 or always):
        dist.barrier()


def max_over_ranks(value, device, always=False):
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not always):
        return float(value)
    t = torch.tensor([float(value)], device="cpu" if dist.get_backend() == "gloo" else device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())
