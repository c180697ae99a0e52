"""The one batch-by-chunk loop of the render paths (matchnerf.launch_chunks) on CPU tensors with a recording callback: every
(batch element, ray) is handed out exactly once, in increasing order, in runs no longer than the limit, through slices that
alias the returned tensors - and no rays means no call."""
import pytest
import torch

from matchnerf_amd.matchnerf import launch_chunks

CHUNK = 7


@pytest.mark.parametrize("batch_size", [1, 2])
@pytest.mark.parametrize("n_rays", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_launch_chunks_hands_every_ray_out_once(batch_size, n_rays):
    calls = []

    def launch(b, first, count, rgb, depth, opacity):
        assert rgb.shape == (count, 3) and depth.shape == (count, 1) and opacity.shape == (count, 1)
        calls.append((b, first, count))
        ray = torch.arange(first, first + count, dtype=torch.float32)[:, None]
        rgb.copy_(1000 * b + ray + torch.tensor([0.0, 0.25, 0.5]))  # a value that names (b, ray, channel)
        depth.copy_(1000 * b + ray + 0.125)
        opacity.copy_(-(1000 * b + ray) - 1)

    out = launch_chunks(batch_size, n_rays, CHUNK, torch.device("cpu"), launch)
    assert sorted(out) == ["depth", "opacity", "rgb"]
    assert out.rgb.shape == (batch_size, n_rays, 3) and out.depth.shape == (batch_size, n_rays, 1)
    assert out.opacity.shape == (batch_size, n_rays, 1)
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" for t in out.values())
    if n_rays == 0:
        assert calls == []
        return
    assert all(1 <= count <= CHUNK for _, _, count in calls)
    for b in range(batch_size):
        mine = [(first, count) for bb, first, count in calls if bb == b]
        assert [first for first, _ in mine] == sorted(first for first, _ in mine)  # increasing within b
        covered = [r for first, count in mine for r in range(first, first + count)]
        assert covered == list(range(n_rays))  # each ray exactly once, none outside
        assert len(mine) == -(-n_rays // CHUNK)  # no launch shorter than it has to be
    assert [b for b, _, _ in calls] == sorted(b for b, _, _ in calls)  # batch elements in order
    # what the callback wrote through its slices is what comes back
    ray = torch.arange(n_rays, dtype=torch.float32)[None, :, None] + 1000 * torch.arange(batch_size, dtype=torch.float32)[:, None, None]
    assert torch.equal(out.rgb, ray + torch.tensor([0.0, 0.25, 0.5]))
    assert torch.equal(out.depth, ray + 0.125)
    assert torch.equal(out.opacity, -ray - 1)

