"""Host logic of the shared encoder (dist.encode_shared) without a GPU: the view / pair partition over the ranks, the ragged
block all_gather over gloo (ranks with nothing to send included), and the guards of encode_shared."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from matchnerf_amd import dist as mdist
from matchnerf_amd.camera import pair_list


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("n_views", [2, 3, 4, 10, 16])
@pytest.mark.parametrize("world", [1, 2, 3, 8, 16])
def test_encoder_partition_covers_every_view_and_pair_once(n_views, world):
    parts = mdist.encoder_partition(n_views, world)
    assert len(parts) == world
    n_pairs = len(pair_list(n_views))
    for k, n in ((0, n_views), (1, n_pairs)):
        shares = [p[k] for p in parts]
        assert all(isinstance(s, range) and s.step == 1 for s in shares)
        assert [i for s in shares for i in s] == list(range(n))     # contiguous, in rank order, each item exactly once
        sizes = [len(s) for s in shares]
        assert max(sizes) - min(sizes) <= 1
    if n_views == 3 and world == 8:
        assert [len(p) for _, p in parts] == [1, 1, 1, 0, 0, 0, 0, 0]
    if n_views == 10 and world == 8:
        assert [len(p) for _, p in parts] == [6, 6, 6, 6, 6, 5, 5, 5]


def _block(rank, n, b=2):
    """deterministic stand-in for a rank's block of pair maps [B, n, 2, 3, 4]: every element a function of its global index"""
    x = torch.arange(b * n * 2 * 3 * 4, dtype=torch.float32).reshape(b, n, 2, 3, 4)
    return x * 0.5 + 1000.0 * rank - 7.0 * torch.arange(b, dtype=torch.float32).reshape(b, 1, 1, 1, 1)


def _worker(rank, world, port, n_items, q):
    try:
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        r, w, _ = mdist.init_from_env(backend="gloo")
        counts = [mdist.shard_range(n_items, i, w)[1] for i in range(w)]
        want = torch.cat([_block(i, counts[i]) for i in range(w)], 1)
        mine = _block(r, counts[r])
        got = mdist.gather_blocks(mine, counts, dim=1)
        ok = torch.equal(got, want) and got.shape == (2, n_items, 2, 3, 4)
        ok = ok and torch.equal(mdist.gather_blocks(mine, dim=1), want)          # counts exchanged first
        flat = mdist.gather_blocks(mine.movedim(1, 0).contiguous(), counts)  # along the first dimension
        ok = ok and torch.equal(flat, want.movedim(1, 0))
        ok = ok and torch.equal(mdist.gather_tiles(mine[0, :, 0, 0]), want[0, :, 0, 0])
        empty = mdist.gather_blocks(torch.zeros(3, 0, 5), [0] * w, dim=1)    # nothing anywhere
        ok = ok and empty.shape == (3, 0, 5)
        try:  # a count that disagrees with the block: every rank raises, none is left waiting in the collective
            mdist.gather_blocks(mine, [c + (1 if i == w - 1 else 0) for i, c in enumerate(counts)], dim=1)
            ok = False
        except ValueError:
            pass
        mdist.barrier()
        q.put((r, bool(ok)))
        torch.distributed.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))


def _run(world, n_items):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_items, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=120) for _ in procs), key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    return res


@pytest.mark.parametrize("world,n_items", [(2, 3), (2, 1), (8, 3), (8, 45), (8, 10)])
def test_ragged_block_gather_reassembles_exactly(world, n_items):
    res = _run(world, n_items)
    if any(isinstance(r[1], str) for r in res):
        # a worker died with an EXCEPTION (rendezvous port taken between _free_port() and init_process_group, ...): transport
        # trouble, not a result - one more attempt on a fresh port.  A mismatch is never retried.
        print("retrying after worker exception:", res)
        res = _run(world, n_items)
    assert res == [(r, True) for r in range(world)], res


class _FakeModel:
    """what encode_shared reads from a MatchNeRF without a process group"""
    n_src_views = 3

    def __init__(self):
        from matchnerf_amd.edict import EasyDict
        self.opts = EasyDict(encoder=EasyDict(attn_splits_list=[2], wo_self_attn=False))
        self.calls = []

    def get_img_feat(self, imgs, attn_splits_list=None, cur_n_src_views=3):
        self.calls.append((tuple(imgs.shape), attn_splits_list, cur_n_src_views))
        return ["maps0", "maps1"]


def test_encode_shared_without_a_group_is_get_img_feat():
    model = _FakeModel()
    with torch.no_grad():
        assert mdist.encode_shared(model, torch.zeros(1, 4, 3, 8, 8)) == ["maps0", "maps1"]
    assert model.calls == [((1, 4, 3, 8, 8), [2], 3)]


def test_encode_shared_refuses_autograd():
    model = _FakeModel()
    with torch.enable_grad(), pytest.raises(RuntimeError, match="inference only"):
        mdist.encode_shared(model, torch.zeros(1, 3, 3, 8, 8))
    assert model.calls == []


def test_sharded_renders_refuse_an_unknown_encoder_mode():
    from matchnerf_amd.edict import EasyDict
    batch = EasyDict(images=torch.zeros(1, 4, 3, 8, 8))
    with pytest.raises(ValueError, match="encoder="):
        mdist.render_frame_sharded(_FakeModel(), batch, encoder="broadcast")
    with pytest.raises(ValueError, match="encoder="):
        mdist.render_views_sharded(_FakeModel(), batch, [], encoder="broadcast")
