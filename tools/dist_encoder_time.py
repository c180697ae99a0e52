"""Encoder shares of sharded rendering: what ``encoder="shared"`` (dist.encode_shared) saves against ``"recompute"``.

One GPU, no process group (``python tools/dist_encoder_time.py``): at BASELINE config[1] (3 views, 512x640) and config[4]
(10 views, 512x640) it times the whole encoder (``model.get_img_feat``) and, for world sizes 2, 3 and 8, every rank's share
(``GMFlow.backbone_tokens`` on its views + ``GMFlow.pair_maps`` on its pairs, ``dist.encoder_partition``) run in turn in this
one process, and prints the bytes each all-gather of ``encode_shared`` moves.  One JSON line per (config, world).

Under torchrun on a multi-GPU node (``torchrun --nproc-per-node N tools/dist_encoder_time.py``): every rank prints its encoder,
map-gather, render and tile-gather times of ``render_frame_sharded`` (row bands of the config[1] frame) for both modes.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from matchnerf_amd import dist as mdist  # noqa: E402
from matchnerf_amd.camera import pair_list  # noqa: E402

CONFIGS = (("config[1]", 3, 512, 640), ("config[4]", 10, 512, 640))


def timed(fn, reps, dev):
    """median of ``reps`` host-clock intervals, each closed by a device synchronise, after one warm-up call -> (ms, result)"""
    out = fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], out


def gather_bytes(model, images, world):
    """bytes of the token gather and of the two map gathers: what every rank receives, and what the padded collective moves"""
    b, v, _, hh, ww = images.shape
    h, w = hh // 8, ww // 8
    up = 2 ** model.feat_enc.featup_net.n_blocks
    parts = mdist.encoder_partition(v, world)
    per_view = b * h * w * 128 * 4
    per_pair = b * 2 * (h * w + up * h * up * w) * 128 * 4
    return dict(tokens_bytes=v * per_view, maps_bytes=len(pair_list(v)) * per_pair,
                tokens_padded_bytes=world * max(len(vs) for vs, _ in parts) * per_view,
                maps_padded_bytes=world * max(len(ps) for _, ps in parts) * per_pair)


def one_gpu(reps, worlds):
    dev = torch.device("cuda:0")
    for name, n_views, height, width in CONFIGS:
        _, model, _ = bench.build_model(dev, n_views)
        _, batch = bench.make_batch(dev, 0, height, width, n_views)
        images = batch.images[:, :n_views]
        enc, splits, wo = model.feat_enc, model.opts.encoder.attn_splits_list, model.opts.encoder.wo_self_attn
        with torch.no_grad():
            full_ms, _ = timed(lambda: model.get_img_feat(images, cur_n_src_views=n_views), reps, dev)
            tok = enc.backbone_tokens(images, None, splits)
            for world in worlds:
                ranks = []
                for views, pairs in mdist.encoder_partition(n_views, world):
                    bb_ms = timed(lambda: enc.backbone_tokens(images, views, splits), reps, dev)[0] if len(views) else 0.0
                    pr_ms = timed(lambda: enc.pair_maps(tok, pairs, splits, wo), reps, dev)[0] if len(pairs) else 0.0
                    ranks.append(dict(views=len(views), pairs=len(pairs), backbone_ms=round(bb_ms, 3), pairs_ms=round(pr_ms, 3),
                                      share_ms=round(bb_ms + pr_ms, 3)))
                print(json.dumps(dict(config=name, n_views=n_views, frame=[height, width], world=world,
                                      full_encoder_ms=round(full_ms, 3), max_share_ms=max(r["share_ms"] for r in ranks),
                                      ranks=ranks, **gather_bytes(model, images, world))), flush=True)
        del model, batch, images, tok
        torch.cuda.empty_cache()


def multi_gpu(reps):
    """Per-rank phases of render_frame_sharded at config[1] for both encoder modes (run under torchrun)."""
    rank, world, dev = mdist.init_from_env()
    _, model, _ = bench.build_model(dev)
    _, batch = bench.make_batch(dev, 0)
    images = batch.images[:, :model.n_src_views]
    tgt_pose, ref_poses = model.extract_poses(batch)
    enc, splits, wo = model.feat_enc, model.opts.encoder.attn_splits_list, model.opts.encoder.wo_self_attn
    b, v, _, h, w = images.shape
    parts = mdist.encoder_partition(v, world)
    views, pairs = parts[rank]
    first, n = mdist.shard_rows(h, w, rank, world)

    def phase(fn):
        mdist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    with torch.no_grad():
        for mode in ("recompute", "shared"):
            rows = []
            for _ in range(reps + 1):
                t = {}
                if mode == "recompute":
                    t["encoder_ms"], feats = phase(lambda: model.get_img_feat(images, cur_n_src_views=v))
                    t["map_gather_ms"] = 0.0
                else:
                    bb_ms, tok = phase(lambda: enc.backbone_tokens(images, views, splits))
                    tg_ms, tok = phase(lambda: mdist.gather_blocks(tok, [len(x) for x, _ in parts], dim=1))
                    pr_ms, maps = phase(lambda: enc.pair_maps(tok, pairs, splits, wo))
                    mg_ms, feats = phase(lambda: [mdist.gather_blocks(m, [len(p) for _, p in parts], dim=1).contiguous()
                                                  for m in maps])
                    t["encoder_ms"], t["map_gather_ms"] = bb_ms + pr_ms, tg_ms + mg_ms
                t["render_ms"], out = phase(lambda: model.render(model.opts, tgt_pose, ray_range=(first, n), mode="test",
                                                                 ref_poses=ref_poses, ref_images=images, ref_feats_list=feats))
                tile = torch.cat([out.rgb, out.depth, out.opacity], -1).permute(1, 0, 2).reshape(n, b * 5)
                t["tile_gather_ms"], _ = phase(lambda: mdist.gather_tiles(
                    tile, [mdist.shard_rows(h, w, r, world)[1] for r in range(world)]))
                rows.append(t)
            med = {k: round(sorted(r[k] for r in rows[1:])[len(rows[1:]) // 2], 3) for k in rows[0]}
            print(json.dumps(dict(rank=rank, world=world, encoder=mode, views=len(views), pairs=len(pairs), **med)), flush=True)
    mdist.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 3, 8])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dist_encoder_time.py times the encoder on a GPU; none is visible")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        multi_gpu(args.reps)
    else:
        one_gpu(args.reps, args.worlds)


if __name__ == "__main__":
    main()
