"""render_frame_sharded at a target grid of its own: two ranks on one GPU (MNERF_FORCE_DEVICE=0, gloo transport - the pattern of
tests/test_dist_gpu.py) split the rows of a 35 x 53 target of 32 x 48 source views (an odd row count: bands of 18 and 17 rows, the
cut inside a 4-row tile band) and gather the frame; it must have the bits of the unsharded frame, with and without supersampling."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SRC_HW, TGT_HW = (32, 48), (35, 53)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), MNERF_FORCE_DEVICE="0", MNERF_DIST_BACKEND="gloo")
        from matchnerf_amd import dist as mdist, options, synthetic as syn
        from matchnerf_amd.edict import EasyDict
        from matchnerf_amd.models import models_dict
        r, w, dev = mdist.init_from_env()
        opt = options.load_options("configs/test.yaml", verbose=False)
        opt.device = str(dev)
        opt.nerf.sample_intvs = 32
        opt.nerf.render_hw = list(TGT_HW)  # the option path: the batch's target camera resized to the grid
        model = models_dict[opt.model](opt).to(dev).eval()
        model.load_state_dict(syn.to_torch(syn.seeded_state_dict(syn.state_dict_spec(), 1), dev))
        scene = syn.make_scene(SRC_HW[0], SRC_HW[1], 3, seed=13)
        batch = EasyDict({k: torch.from_numpy(v).to(dev) for k, v in scene.items()})
        n = TGT_HW[0] * TGT_HW[1]
        with torch.no_grad():
            # ONE set of feature maps for every rank and both renders (library convolutions are not bitwise reproducible across
            # processes; the claim under test is about the sharded render and the gather)
            feats = model.get_img_feat(batch.images[:, :3], cur_n_src_views=3)
            for f in feats:
                host = f.cpu()
                torch.distributed.broadcast(host, src=0)
                f.copy_(host.to(dev))
            model.get_img_feat = lambda *a, **k: feats
            ok = True
            for ssaa in (1, 2):
                opt.nerf.render_ssaa = ssaa
                sharded = mdist.render_frame_sharded(model, batch)
                whole = model(EasyDict(dict(batch)), mode="test")
                ok = ok and all(torch.equal(sharded[k], whole[k]) for k in ("rgb", "depth", "opacity"))
                ok = ok and sharded.rgb.shape == (1, n, 3) and sharded.depth.shape == (1, n, 1)
                ok = ok and bool(torch.isfinite(sharded.rgb).all())
        mdist.barrier()
        q.put((r, bool(ok), float(whole.rgb.mean())))
        torch.distributed.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        q.put((rank, False, repr(e)))


def _run_ranks(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    return res


def test_sharded_frame_at_a_target_grid_is_bit_identical():
    res = _run_ranks(2)
    if any(isinstance(r[2], str) for r in res):
        # a worker died with an EXCEPTION (rendezvous port taken between _free_port() and init_process_group, ...): transport
        # trouble, not a result - one more attempt on a fresh port.  A frame mismatch is never retried.
        print("retrying after worker exception:", res)
        res = _run_ranks(2)
    assert [r[:2] for r in res] == [(0, True), (1, True)], res
    assert len({r[2] for r in res}) == 1
